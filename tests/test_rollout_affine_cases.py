"""The table of tests/rollout_affine_cases.py pinned on the CPU oracle, and the recursion of tests/rollout_affine_ref.py
(include_ext5/mpcqp_rollout_affine.h) against central differences of the stepped closed loop on the oracle, in a direction of d0 and one of the
whole schedule -- with the step and the tolerance of tests/test_rollout_cases.py.  No GPU needed."""
import numpy as np
import pytest

import rollout_affine_cases as ac
import rollout_affine_ref as ar
import rollout_cases as rc


def test_the_table_has_the_cases_and_two_instances_each():
    assert set(ac.NAMES) == {'first', 'held', 'hard', 'headline', 'nb32_soft'}
    shapes = {n: (rc.CASES[n]['nx'], rc.CASES[n]['nu'], rc.CASES[n]['Np']) for n in ac.NAMES}
    assert shapes == dict(first=(4, 2, 10), held=(5, 3, 12), hard=(7, 7, 4), headline=(12, 4, 30), nb32_soft=(20, 5, 6))
    assert rc.CASES['held']['Nc'] == 6 and not rc.CASES['hard']['soft']
    assert ac.combos() == [('1', 1), ('1', 2), ('Np', 1), ('Np', 2)]
    for n in ac.NAMES:
        assert len(set(ac.SEEDS[n])) >= 2 and max(ac.SEEDS[n]) < 100, n
    for n in ac.SCHEDULED:
        assert n in ac.NAMES


@pytest.mark.parametrize('rows,hold', ac.combos())
@pytest.mark.parametrize('name,seed', ac.triples())
def test_every_listed_seed_meets_the_conditions(name, seed, rows, hold):
    kw, attrs = rc.draw(name, seed)
    d0, dt = ac.terms(name, seed, rows, hold)
    assert d0.shape == (ac.nrows(name, rows), rc.CASES[name]['nx']) and dt.shape[0] == ac.nent(name, hold)
    tape, X, U, scaling = ac.oracle_rollout(kw, attrs, rc.CASES[name]['K'], d0, dt, hold, with_last=True)
    f = ac.tape_facts(kw, attrs, tape, scaling, ac.slots(d0, dt), hold)
    print('ROLLOUT_AFFINE_CASE %s/%d rows %s hold %d: n_ineq %s n_weak %s same %s' % (name, seed, rows, hold, f['n_ineq'].tolist(), f['n_weak'].tolist(),
                                                                                 f['same'].astype(int).tolist()))
    assert f['solved'].all(), (name, seed, f['solved'])
    assert (f['n_weak'] == 0).all(), (name, seed, f['n_weak'])
    assert f['n_ineq'].max() >= 1, (name, seed, f['n_ineq'])
    assert f['same'].any() and not f['same'].all(), (name, seed, f['same'])


# ---- the recursion against central differences of the stepped loop ---------------------------------------------------------------------
H = 1e-6                   # (tests/test_rollout_cases.py)
EPS_FD = 1e-10


def _loss(kw, attrs, K, Gx, Gu, d0, dt, hold, w):
    _, X, U, _ = ac.oracle_rollout(kw, attrs, K, d0, dt, hold, w=w, eps=EPS_FD)
    return float((Gx * X).sum() + (Gu * U).sum())


@pytest.mark.parametrize('rows,hold', ac.combos())
def test_the_restatement_against_central_differences(rows, hold):
    """L = sum_k <Gx[k], x_k> + sum_k <Gu[k], u_k> of the stepped loop with the term: rollout_affine_ref's d_slots against (L(d + h v) - L(d - h v)) / 2h
    for a direction v of d0 alone and one of the whole schedule, and lam[0] against a direction of x0, within 1e-4 max(1, |fd|_inf)."""
    name, seed = 'first', ac.SEEDS['first'][0]
    c = rc.CASES[name]
    K, nx, nu = c['K'], c['nx'], c['nu']
    kw, attrs = rc.draw(name, seed)
    kw = ar.adjoint_model_ref.full_kwargs(kw)
    rng = np.random.default_rng(60 + hold)
    Gx, Gu = rng.standard_normal((K + 1, nx)), rng.standard_normal((K, nu))
    w = 0.01 * rng.standard_normal((K, nx))
    d0, dt = ac.terms(name, seed, rows, hold)
    tape, X, U, (D, E, cs) = ac.oracle_rollout(kw, attrs, K, d0, dt, hold, w=w, eps=EPS_FD)
    f = ac.tape_facts(kw, attrs, tape, (D, E, cs), ac.slots(d0, dt), hold)
    assert f['solved'].all() and (f['n_weak'] == 0).all(), (f['solved'], f['n_weak'])      # (nothing excluded: no kink on the way)
    ref = ar.sweep(kw, attrs, tape, ac.slots(d0, dt), hold, [dict(Ad=kw['Ad'], Bd=kw['Bd'], D=D, E=E, c=cs)], 0, Gx, Gu)
    assert (ref['status'] == 1).all()
    v0, vt, vx = rng.standard_normal(d0.shape), rng.standard_normal(dt.shape), rng.standard_normal(nx)
    v0, vt, vx = v0 / np.linalg.norm(v0), vt / np.linalg.norm(vt), vx / np.linalg.norm(vx)

    def fd(a0, at, ax):
        vals = []
        for sgn in (1.0, -1.0):
            k2 = dict(kw, x0=kw['x0'] + sgn * H * ax * vx)
            vals.append(_loss(k2, attrs, K, Gx, Gu, d0 + sgn * H * a0 * v0, dt + sgn * H * at * vt, hold, w))
        return (vals[0] - vals[1]) / (2 * H)

    checks = [('d0', float((ref['d_slots'][0] * v0).sum()), fd(1.0, 0.0, 0.0)),
              ('schedule', float((ref['d_slots'][1:] * vt).sum()), fd(0.0, 1.0, 0.0)),
              ('x0', float(ref['lam'][0] @ vx), fd(0.0, 0.0, 1.0))]
    scale = max(1.0, max(abs(v) for _, _, v in checks))
    for n, got, want in checks:
        print('ROLLOUT_AFFINE_FD rows %s hold %d %s: ref %+.6e fd %+.6e' % (rows, hold, n, got, want))
    for n, got, want in checks:
        assert abs(got - want) <= 1e-4 * scale, (n, got, want)
    assert max(abs(v) for _, _, v in checks) > 1e-3        # (the differences are not all in the noise)
    if hold == 1:                                          # the last entry's only solve is the one for x_K, which is on no tape
        assert not ref['d_slots'][-1].any() and ref['d_slots'][1].any()
