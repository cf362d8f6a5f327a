"""The table of tests/rollout_tv_est_cases.py pinned on the CPU oracle, and the recursion of tests/rollout_tv_est_ref.py
(include_ext2/mpcqp_rollout_tv_est.h) against central differences of the output-feedback loop stepped under the schedule on the oracle.
No GPU needed."""
import numpy as np
import pytest

import rollout_cases as rc
import rollout_est_cases as ec
import rollout_tv_cases as tc
import rollout_tv_est_cases as xc
import rollout_tv_est_ref as xr

_tapes = {}


def _rollout(name, seed, hold):
    """The oracle's K + 1 solves of one (case, seed, hold), made once."""
    key = (name, seed, hold)
    if key not in _tapes:
        i = xc.instance(name, seed, hold)
        tape, X, XH, Y, U, slots = xc.oracle_rollout(i['kw'], i['attrs'], i['K'], i['Adt'], i['Bdt'], hold, i['C'], i['Lt'], i['x_true0'], v=i['v'], w=i['w'],
                                                     with_last=True)
        _tapes[key] = (i, tape, slots)
    return _tapes[key]


def test_the_table():
    assert xc.HOLDS == (1, 2) and xc.NOISE == 0.01
    assert xc.SEEDS == dict(first=(0, 3, 4, 6), held=(3, 5, 7), hard=(5, 7, 8), headline=(0, 11), nb32_soft=(4, 8, 24))
    for name in xc.NAMES:                                  # every instance is one of the unscheduled estimator table, under the schedule of the scheduled one
        assert set(xc.SEEDS[name]) <= set(ec.SEEDS[name]) and name in tc.NAMES
    shapes = {n: (rc.CASES[n]['nx'], rc.CASES[n]['nu'], rc.CASES[n]['Np'], rc.CASES[n]['K']) for n in xc.NAMES}
    assert shapes == dict(first=(4, 2, 10, 6), held=(5, 3, 12, 4), hard=(7, 7, 4, 4), headline=(12, 4, 30, 3), nb32_soft=(20, 5, 6, 3))


def test_the_gains_differ_between_entries():
    i = xc.instance(xc.FIRST, 0, 2)
    assert i['Lt'].shape == (3, 4, 2)
    d = max(np.abs(i['Lt'][e] - i['Lt'][0]).max() for e in (1, 2))
    print('ROLLOUT_TV_EST_GAINS first/0 hold 2: max |L_e - L_0| = %.3e' % d)
    assert d > 1e-4


@pytest.mark.parametrize('name,seed,hold', xc.triples())
def test_every_listed_seed_meets_the_conditions(name, seed, hold):
    i, tape, slots = _rollout(name, seed, hold)
    f = tc.tape_facts(i['kw'], i['attrs'], tape, slots, hold)
    print('ROLLOUT_TV_EST_CASE %s/%d hold %d: n_ineq %s n_weak %s same %s' % (name, seed, hold, f['n_ineq'].tolist(), f['n_weak'].tolist(), f['same'].astype(int).tolist()))
    assert len(tape) == i['K'] + 1 and len(slots) == tc.nseg(name, hold) + 1
    assert f['solved'].all(), (name, seed, hold, f['solved'])
    assert (f['n_weak'] == 0).all(), (name, seed, hold, f['n_weak'])
    assert f['n_ineq'].max() >= 2, (name, seed, hold, f['n_ineq'])
    assert f['same'].any() and not f['same'].all(), (name, seed, hold, f['same'])


# ---- the recursion against central differences of the stepped loop ---------------------------------------------------------------------
FD_SEEDS = (0, 3)
HOLD = 2
H = 1e-6
EPS_FD = 1e-10


@pytest.mark.parametrize('own_plant', (False, True), ids=('plant_follows', 'plant_given'))
@pytest.mark.parametrize('seed', FD_SEEDS)
def test_the_restatement_against_central_differences(seed, own_plant):
    """L = sum <Gx[k], x_k> + <Gxh[k], xh_k> + <Gu[k], u_k> + <Gy[k], y_k> of the loop stepped under the schedule with a gain per entry:
    rollout_tv_est_ref against (L(p + h) - L(p - h)) / 2h in entries of Ad_traj[e] (solve + estimator paths, + the plant's where it follows),
    Bd_traj[e] and L_traj[e], of C, xhat0, x0 and the Ad the loop began under (slot 0), within 1e-4 max(1, |fd|_inf) -- H, EPS_FD and the
    bound of tests/test_rollout_tv_cases.py."""
    i = xc.instance(xc.FIRST, seed, HOLD)
    K, attrs = i['K'], i['attrs']
    kw = xr.adjoint_model_ref.full_kwargs(i['kw'])
    nx, nu = kw['Bd'].shape
    ny = i['C'].shape[0]
    rng = np.random.default_rng(70 + seed)
    Gx, Gxh, Gu, Gy = rng.standard_normal((K + 1, nx)), rng.standard_normal((K + 1, nx)), rng.standard_normal((K, nu)), rng.standard_normal((K, ny))
    Ap = Bp = None
    if own_plant:
        Ap = kw['Ad'] + 0.02 * rng.standard_normal((nx, nx)); Bp = kw['Bd'] + 0.02 * rng.standard_normal((nx, nu))

    def roll(k2, p):
        return xc.oracle_rollout(k2, attrs, K, p['Ad'], p['Bd'], HOLD, p['C'], p['L'], p['xt'], v=i['v'], w=i['w'], Ap=Ap, Bp=Bp, eps=EPS_FD)
    base = dict(Ad=i['Adt'], Bd=i['Bdt'], C=i['C'], L=i['Lt'], xt=i['x_true0'])
    tape, X, XH, Y, U, slots = roll(kw, base)
    f = tc.tape_facts(kw, attrs, tape, slots, HOLD)
    assert f['solved'].all() and (f['n_weak'] == 0).all(), (f['solved'], f['n_weak'])      # (nothing excluded: no kink on the way)
    ref = xr.sweep(kw, attrs, tape, slots, HOLD, i['C'], i['Lt'], Gx, Gxh, Gu, Gy, Ap=Ap, Bp=Bp)
    assert (ref['status'] == 1).all()

    def fd(change):
        vals = []
        for sgn in (1.0, -1.0):
            k2 = {k: (np.array(v, dtype=float) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
            p = {k: np.array(v, dtype=float) for k, v in base.items()}
            change(k2, p, sgn * H)
            _, X2, XH2, Y2, U2, _ = roll(k2, p)
            vals.append(float((Gx * X2).sum() + (Gxh * XH2).sum() + (Gu * U2).sum() + (Gy * Y2).sum()))
        return (vals[0] - vals[1]) / (2 * H)

    def bump(which, idx):
        def change(k2, p, h):
            (k2 if which in ('x0', 'Ad0') else p)[{'x0': 'x0', 'Ad0': 'Ad'}.get(which, which)][idx] += h
        return change
    plant = 0.0 if own_plant else 1.0
    checks = []
    for (e, a, b) in ((1, 0, 0), (1, 1, 2), (0, 3, 1), (2, 2, 3)):
        want = ref['Ad_slots'][e + 1][a, b] + ref['Ae_entries'][e][a, b] + plant * ref['Ap_entries'][e][a, b]
        checks.append(('Ad_traj[%d][%d,%d]' % (e, a, b), want, fd(bump('Ad', (e, a, b)))))
    for (e, a, b) in ((0, 0, 1), (1, 2, 0)):
        want = ref['Bd_slots'][e + 1][a, b] + ref['Be_entries'][e][a, b] + plant * ref['Bp_entries'][e][a, b]
        checks.append(('Bd_traj[%d][%d,%d]' % (e, a, b), want, fd(bump('Bd', (e, a, b)))))
    for (e, a, b) in ((0, 0, 0), (1, 3, 1), (2, 1, 0)):
        checks.append(('L_traj[%d][%d,%d]' % (e, a, b), ref['L_entries'][e][a, b], fd(bump('L', (e, a, b)))))
    for (a, b) in ((0, 0), (1, 3)):
        checks.append(('C[%d,%d]' % (a, b), ref['C'][a, b], fd(bump('C', (a, b)))))
    for j in (0, nx - 1):
        checks.append(('xhat0[%d]' % j, ref['eta'][0][j], fd(bump('x0', j))))
        checks.append(('x0[%d]' % j, ref['lam'][0][j], fd(bump('xt', j))))
    for (a, b) in ((0, 0), (2, 3)):                         # the model the loop began under: the solve of entry 0 alone (plant and estimator never have it)
        checks.append(('Ad slot 0 [%d,%d]' % (a, b), ref['Ad_slots'][0][a, b], fd(bump('Ad0', (a, b)))))
    scale = max(1.0, max(abs(v) for _, _, v in checks))
    for name, got, want in checks:
        print('ROLLOUT_TV_EST_FD seed %d %s %s: ref %+.6e fd %+.6e' % (seed, 'own plant' if own_plant else 'plant follows', name, got, want))
    for name, got, want in checks:
        assert abs(got - want) <= 1e-4 * scale, (name, got, want)
    assert max(abs(v) for _, _, v in checks) > 1e-3         # (the differences are not all in the noise)
