"""The table of tests/rollout_cases.py pinned on the CPU oracle, and the recursion of tests/rollout_ref.py (include/mpcqp_rollout.h) against
central differences of the stepped closed loop on the oracle.  No GPU needed."""
import numpy as np
import pytest

import rollout_cases as rc
import rollout_ref as rr

_tapes = {}


def _rollout(name, seed):
    """The oracle's K + 1 solves of one (case, seed), made once."""
    if (name, seed) not in _tapes:
        kw, attrs = rc.draw(name, seed)
        tape, X, U, scaling = rc.oracle_rollout(kw, attrs, rc.CASES[name]['K'], xrefs=rc.xref_traj(name, seed), with_last=True)
        _tapes[(name, seed)] = (kw, attrs, tape, X, U, scaling)
    return _tapes[(name, seed)]


def test_the_table_covers_the_paths():
    shapes = {(c['nx'], c['nu'], c['Np'], c['Nc'], c['soft'], c['tv']) for c in rc.CASES.values()}
    for want in ((4, 2, 10, 10, True, False), (4, 2, 10, 10, True, True), (20, 5, 6, 6, True, False), (5, 3, 12, 6, True, False),
                 (7, 7, 4, 4, False, False), (4, 2, 100, 100, True, False), (36, 6, 4, 4, True, False), (64, 5, 3, 3, True, False), (12, 4, 30, 30, True, False)):
        assert want in shapes, want
    for name, c in rc.CASES.items():
        assert len(c['seeds']) >= 2 and 2 <= c['K'] <= 6, name
        assert max(c['seeds']) < 100                       # (random_lti(7200 + seed): clear of the 7100 block of tests/adjoint_cases.py)


@pytest.mark.parametrize('name,seed', rc.pairs())
def test_every_listed_seed_meets_the_conditions(name, seed):
    kw, attrs, tape, X, U, scaling = _rollout(name, seed)
    f = rc.tape_facts(kw, attrs, tape, scaling)
    print('ROLLOUT_CASE %s/%d: n_ineq %s n_weak %s same %s' % (name, seed, f['n_ineq'].tolist(), f['n_weak'].tolist(), f['same'].astype(int).tolist()))
    assert f['solved'].all(), (name, seed, f['solved'])
    assert (f['n_weak'] == 0).all(), (name, seed, f['n_weak'])
    assert f['n_ineq'].max() >= 2, (name, seed, f['n_ineq'])
    assert f['same'].any() and not f['same'].all(), (name, seed, f['same'])


def test_the_first_case_reuses_a_factor_within_its_tape():
    """What the reuse test on the device needs: an instance whose K tape entries take more than one and fewer than K factorizations."""
    K = rc.CASES[rc.FIRST]['K']
    counts = []
    for seed in rc.CASES[rc.FIRST]['seeds']:
        kw, attrs, tape, X, U, scaling = _rollout(rc.FIRST, seed)
        same = rc.tape_facts(kw, attrs, tape[:K], scaling)['same']
        counts.append(1 + int(np.count_nonzero(~same)))
    assert any(1 < n < K for n in counts), counts


# ---- the recursion against central differences of the stepped loop ---------------------------------------------------------------------
FD_SEEDS = (0, 5)          # random_lti(7200 / 7205, ...): one loop that keeps changing its active set, one that does not settle before step 5
H = 1e-6
EPS_FD = 1e-10


def _loss(kw, attrs, K, Gx, Gu, Ap, Bp, w):
    _, X, U, _ = rc.oracle_rollout(kw, attrs, K, Ap=Ap, Bp=Bp, w=w, eps=EPS_FD)
    return float((Gx * X).sum() + (Gu * U).sum())


@pytest.mark.parametrize('own_plant', (False, True), ids=('plant_is_model', 'plant_given'))
@pytest.mark.parametrize('seed', FD_SEEDS)
def test_the_restatement_against_central_differences(seed, own_plant):
    """L = sum_k <Gx[k], x_k> + sum_k <Gu[k], u_k> of the stepped loop: rollout_ref against (L(p + h) - L(p - h)) / 2h in entries of x0, u_{-1},
    uref, Ad, Bd, Qx and w[k], within 1e-4 max(1, |fd|_inf) (the bound of tests/test_gpu_adjoint.py for central differences)."""
    c = rc.CASES[rc.FIRST]
    K, nx, nu = c['K'], c['nx'], c['nu']
    kw, attrs = rc.draw(rc.FIRST, seed)
    kw = rr.adjoint_model_ref.full_kwargs(kw)
    rng = np.random.default_rng(40 + seed)
    Gx, Gu = rng.standard_normal((K + 1, nx)), rng.standard_normal((K, nu))
    w = 0.01 * rng.standard_normal((K, nx))
    Ap = Bp = None
    if own_plant:
        Ap = kw['Ad'] + 0.02 * rng.standard_normal((nx, nx)); Bp = kw['Bd'] + 0.02 * rng.standard_normal((nx, nu))
    tape, X, U, (D, E, cs) = rc.oracle_rollout(kw, attrs, K, Ap=Ap, Bp=Bp, w=w, eps=EPS_FD)
    f = rc.tape_facts(kw, attrs, tape, (D, E, cs))
    assert f['solved'].all() and (f['n_weak'] == 0).all(), (f['solved'], f['n_weak'])      # (nothing excluded: no kink on the way)
    ref = rr.sweep(kw, attrs, tape, D, E, cs, Gx, Gu, Ap=Ap, Bp=Bp)
    assert ref['n_solved'] == K and (ref['status'] == 1).all()

    def fd(change):
        vals = []
        for sgn in (1.0, -1.0):
            k2 = {k: (np.array(v, dtype=float) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
            plant = dict(Ap=None if Ap is None else Ap.copy(), Bp=None if Bp is None else Bp.copy(), w=w.copy())
            change(k2, plant, sgn * H)
            vals.append(_loss(k2, attrs, K, Gx, Gu, plant['Ap'], plant['Bp'], plant['w']))
        return (vals[0] - vals[1]) / (2 * H)

    checks = []
    for j in (0, nx - 1):
        checks.append(('x0[%d]' % j, ref['lam'][0][j], fd(lambda k2, p, h, j=j: k2['x0'].__setitem__(j, k2['x0'][j] + h))))
    for j in range(nu):
        checks.append(('um1[%d]' % j, ref['uminus1'][j], fd(lambda k2, p, h, j=j: k2['uminus1'].__setitem__(j, k2['uminus1'][j] + h))))
        checks.append(('uref[%d]' % j, ref['uref'][j], fd(lambda k2, p, h, j=j: k2['uref'].__setitem__(j, k2['uref'][j] + h))))
    for (i, j) in ((0, 0), (1, 2), (3, 1)):
        # the controller's Ad: with the plant equal to the model the same entry moves the plant too (d_Ad + d_Ap)
        want = ref['Ad'][i, j] + (ref['Ap'][i, j] if not own_plant else 0.0)
        checks.append(('Ad[%d,%d]' % (i, j), want, fd(lambda k2, p, h, i=i, j=j: k2['Ad'].__setitem__((i, j), k2['Ad'][i, j] + h))))
    for (i, j) in ((0, 1), (2, 0)):
        want = ref['Bd'][i, j] + (ref['Bp'][i, j] if not own_plant else 0.0)
        checks.append(('Bd[%d,%d]' % (i, j), want, fd(lambda k2, p, h, i=i, j=j: k2['Bd'].__setitem__((i, j), k2['Bd'][i, j] + h))))
    if own_plant:
        checks.append(('Ap[1,1]', ref['Ap'][1, 1], fd(lambda k2, p, h: p['Ap'].__setitem__((1, 1), p['Ap'][1, 1] + h))))
        checks.append(('Bp[2,1]', ref['Bp'][2, 1], fd(lambda k2, p, h: p['Bp'].__setitem__((2, 1), p['Bp'][2, 1] + h))))

    def move_qx(k2, p, h, i, j):                           # a symmetric perturbation: (i, j) and (j, i) together, dL = 2 d_Qx[i, j] h off the diagonal
        k2['Qx'][i, j] += h
        if i != j:
            k2['Qx'][j, i] += h
    for (i, j) in ((0, 0), (1, 2)):
        checks.append(('Qx[%d,%d]' % (i, j), ref['Qx'][i, j] * (1.0 if i == j else 2.0), fd(lambda k2, p, h, i=i, j=j: move_qx(k2, p, h, i, j))))
    for (k, j) in ((0, 1), (K - 2, 3)):
        checks.append(('w[%d][%d]' % (k, j), ref['lam'][k + 1][j], fd(lambda k2, p, h, k=k, j=j: p['w'].__setitem__((k, j), p['w'][k, j] + h))))
    scale = max(1.0, max(abs(v) for _, _, v in checks))
    for name, got, want in checks:
        print('ROLLOUT_FD seed %d %s %s: ref %+.6e fd %+.6e' % (seed, 'own plant' if own_plant else 'model', name, got, want))
    for name, got, want in checks:
        assert abs(got - want) <= 1e-4 * scale, (name, got, want)
    assert max(abs(v) for _, _, v in checks) > 1e-3        # (the differences are not all in the noise)
