"""The table of tests/rollout_tv_cases.py pinned on the CPU oracle, and the recursion of tests/rollout_tv_ref.py
(include_ext/mpcqp_rollout_tv.h) against central differences of the closed loop stepped under the schedule on the oracle.  No GPU needed."""
import numpy as np
import pytest

import rollout_cases as rc
import rollout_tv_cases as tc
import rollout_tv_ref as tr

_tapes = {}


def _rollout(name, seed, hold):
    """The oracle's K + 1 solves of one (case, seed, hold), made once."""
    key = (name, seed, hold)
    if key not in _tapes:
        kw, attrs = rc.draw(name, seed)
        Adt, Bdt = tc.schedule(name, seed, hold)
        tape, X, U, slots = tc.oracle_rollout(kw, attrs, rc.CASES[name]['K'], Adt, Bdt, hold, with_last=True)
        _tapes[key] = (kw, attrs, tape, X, U, slots)
    return _tapes[key]


def test_the_table_is_the_listed_part_of_the_unscheduled_one():
    assert tc.NAMES == ('first', 'headline', 'held', 'hard', 'nb32_soft') and tc.HOLDS == (1, 2) and tc.AMP == 0.03
    for name in tc.NAMES:
        assert tc.SEEDS[name] == rc.CASES[name]['seeds'] and not rc.CASES[name]['tv']
        for hold in tc.HOLDS:
            assert tc.nseg(name, hold) == -(-rc.CASES[name]['K'] // hold)


def test_the_slots_of_solve_and_plant_differ_at_every_boundary_step():
    for hold in (1, 2, 3):
        for k in range(9):
            s, p = tr.sigma(k, hold), 1 + k // hold
            assert (s != p) == (k % hold == 0) and s <= p <= s + 1
    assert [tr.sigma(k, 2) for k in range(6)] == [0, 1, 1, 2, 2, 3]


@pytest.mark.parametrize('name,seed,hold', tc.triples())
def test_every_listed_seed_meets_the_conditions(name, seed, hold):
    kw, attrs, tape, X, U, slots = _rollout(name, seed, hold)
    f = tc.tape_facts(kw, attrs, tape, slots, hold)
    print('ROLLOUT_TV_CASE %s/%d hold %d: n_ineq %s n_weak %s same %s' % (name, seed, hold, f['n_ineq'].tolist(), f['n_weak'].tolist(), f['same'].astype(int).tolist()))
    assert len(slots) == tc.nseg(name, hold) + 1
    assert f['solved'].all(), (name, seed, hold, f['solved'])
    assert (f['n_weak'] == 0).all(), (name, seed, hold, f['n_weak'])
    assert f['n_ineq'].max() >= 2, (name, seed, hold, f['n_ineq'])
    assert f['same'].any() and not f['same'].all(), (name, seed, hold, f['same'])


def test_the_first_case_has_equal_sets_across_an_entry_boundary():
    """Where reuse must not happen: with hold = 2 some instance of 'first' has two consecutive tape entries with equal active sets made under
    different slots."""
    K = rc.CASES[rc.FIRST]['K']
    hits = []
    for seed in tc.SEEDS[rc.FIRST]:
        kw, attrs, tape, X, U, slots = _rollout(rc.FIRST, seed, 2)
        f = tc.tape_facts(kw, attrs, tape[:K], slots, 2)
        hits.append(bool(np.any(f['same'] & (f['slot'][:-1] != f['slot'][1:]))))
    assert any(hits), hits


# ---- the recursion against central differences of the stepped loop ---------------------------------------------------------------------
FD_SEEDS = (0, 5)
HOLD = 2
H = 1e-6
EPS_FD = 1e-10


def _loss(kw, attrs, K, Adt, Bdt, Gx, Gu, Ap, Bp, w):
    _, X, U, _ = tc.oracle_rollout(kw, attrs, K, Adt, Bdt, HOLD, Ap=Ap, Bp=Bp, w=w, eps=EPS_FD)
    return float((Gx * X).sum() + (Gu * U).sum())


@pytest.mark.parametrize('own_plant', (False, True), ids=('plant_follows', 'plant_given'))
@pytest.mark.parametrize('seed', FD_SEEDS)
def test_the_restatement_against_central_differences(seed, own_plant):
    """L = sum_k <Gx[k], x_k> + sum_k <Gu[k], u_k> of the loop stepped under the schedule: rollout_tv_ref against (L(p + h) - L(p - h)) / 2h
    in entries of Ad_traj[1] and Bd_traj[0] (with the plant following: solve path plus plant path; with its own plant: the solve path
    alone), the Ad the loop began under (slot 0), x0 and Qx, within 1e-4 max(1, |fd|_inf) -- H, EPS_FD and the bound of
    tests/test_rollout_cases.py."""
    c = rc.CASES[rc.FIRST]
    K, nx, nu = c['K'], c['nx'], c['nu']
    kw, attrs = rc.draw(rc.FIRST, seed)
    kw = tr.adjoint_model_ref.full_kwargs(kw)
    Adt, Bdt = tc.schedule(rc.FIRST, seed, HOLD)
    rng = np.random.default_rng(60 + seed)
    Gx, Gu = rng.standard_normal((K + 1, nx)), rng.standard_normal((K, nu))
    w = 0.01 * rng.standard_normal((K, nx))
    Ap = Bp = None
    if own_plant:
        Ap = kw['Ad'] + 0.02 * rng.standard_normal((nx, nx)); Bp = kw['Bd'] + 0.02 * rng.standard_normal((nx, nu))
    tape, X, U, slots = tc.oracle_rollout(kw, attrs, K, Adt, Bdt, HOLD, Ap=Ap, Bp=Bp, w=w, eps=EPS_FD)
    f = tc.tape_facts(kw, attrs, tape, slots, HOLD)
    assert f['solved'].all() and (f['n_weak'] == 0).all(), (f['solved'], f['n_weak'])      # (nothing excluded: no kink on the way)
    ref = tr.sweep(kw, attrs, tape, slots, HOLD, Gx, Gu, Ap=Ap, Bp=Bp)
    assert (ref['status'] == 1).all()

    def fd(change):
        vals = []
        for sgn in (1.0, -1.0):
            k2 = {k: (np.array(v, dtype=float) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
            sched = dict(Ad=Adt.copy(), Bd=Bdt.copy())
            change(k2, sched, sgn * H)
            vals.append(_loss(k2, attrs, K, sched['Ad'], sched['Bd'], Gx, Gu, Ap, Bp, w))
        return (vals[0] - vals[1]) / (2 * H)

    plant = 0.0 if own_plant else 1.0
    checks = []
    for (i, j) in ((0, 0), (1, 2), (3, 1)):
        want = ref['Ad_slots'][2][i, j] + plant * ref['Ap_entries'][1][i, j]
        checks.append(('Ad_traj[1][%d,%d]' % (i, j), want, fd(lambda k2, s, h, i=i, j=j: s['Ad'].__setitem__((1, i, j), s['Ad'][1, i, j] + h))))
    for (i, j) in ((0, 1), (2, 0)):
        want = ref['Bd_slots'][1][i, j] + plant * ref['Bp_entries'][0][i, j]
        checks.append(('Bd_traj[0][%d,%d]' % (i, j), want, fd(lambda k2, s, h, i=i, j=j: s['Bd'].__setitem__((0, i, j), s['Bd'][0, i, j] + h))))
    for (i, j) in ((0, 0), (2, 3)):                         # the model the loop began under: the solve of entry 0 alone (the plant never has it)
        checks.append(('Ad slot 0 [%d,%d]' % (i, j), ref['Ad_slots'][0][i, j], fd(lambda k2, s, h, i=i, j=j: k2['Ad'].__setitem__((i, j), k2['Ad'][i, j] + h))))
    for j in (0, nx - 1):
        checks.append(('x0[%d]' % j, ref['lam'][0][j], fd(lambda k2, s, h, j=j: k2['x0'].__setitem__(j, k2['x0'][j] + h))))

    def move_qx(k2, s, h, i, j):                            # a symmetric perturbation: (i, j) and (j, i) together, dL = 2 d_Qx[i, j] h off the diagonal
        k2['Qx'][i, j] += h
        if i != j:
            k2['Qx'][j, i] += h
    for (i, j) in ((0, 0), (1, 2)):
        checks.append(('Qx[%d,%d]' % (i, j), ref['Qx'][i, j] * (1.0 if i == j else 2.0), fd(lambda k2, s, h, i=i, j=j: move_qx(k2, s, h, i, j))))
    scale = max(1.0, max(abs(v) for _, _, v in checks))
    for name, got, want in checks:
        print('ROLLOUT_TV_FD seed %d %s %s: ref %+.6e fd %+.6e' % (seed, 'own plant' if own_plant else 'plant follows', name, got, want))
    for name, got, want in checks:
        assert abs(got - want) <= 1e-4 * scale, (name, got, want)
    assert max(abs(v) for _, _, v in checks) > 1e-3         # (the differences are not all in the noise)
