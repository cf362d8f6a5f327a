"""The table of tests/bounds_cases.py pinned on the CPU oracle, and the restatement tests/bounds_ref.py (include/mpcqp_adjoint_bounds.h)
against central differences of the stepped closed loop on the oracle.  No GPU needed."""
import numpy as np
import pytest

import adjoint_ref as ar
import adjoint_model_ref as am
import bounds_cases as bc
import bounds_ref as br
import rollout_cases as rc
import rollout_ref as rr

EPS = 1e-9
H = 1e-6                   # the step and the solver tolerance of the central differences of tests/test_rollout_cases.py: the same
EPS_FD = 1e-10             # solver, the same conditioning
WEAK_TOL = 1e-6            # the device's default (include/mpcqp_adjoint.h)
_made = {}


def _single(name):
    """One SINGLE entry solved by the oracle, made once: (kw, attrs, the argument list of adjoint_ref.adjoint, status)."""
    if name not in _made:
        import util
        kw, attrs = bc.single(name)
        K = util.oracle_controller(kw, attrs, eps=EPS, setup=True, quiet=True, max_iter=4000000)
        x, z, y, _ = K.prob.iterate_state()
        D, E, c = K.prob.scaling()
        _made[name] = (kw, attrs, (K.P, K.A, np.asarray(K.l, dtype=float), np.asarray(K.u, dtype=float), x, z, y, D, E, c), K.res.info.status)
    return _made[name]


def _tape(key):
    """The oracle's K solves of a ROLLOUT pair or a LOOPS name, made once: (kw, attrs, tape, scaling)."""
    if key not in _made:
        if isinstance(key, tuple):
            kw, attrs = rc.draw(*key)
            K = rc.CASES[key[0]]['K']
        else:
            kw, attrs = bc.loop(key)
            K = bc.LOOPS[key]['K']
        tape, _, _, scaling = rc.oracle_rollout(kw, attrs, K, eps=EPS)
        _made[key] = (kw, attrs, tape, scaling)
    return _made[key]


def _sets_of_tape(key):
    kw, attrs, tape, (D, E, c) = _tape(key)
    out = []
    for e in tape:
        (P, _, A, l, u), _ = am.build(rr.entry_kwargs(kw, e), attrs)
        out.append(bc.active_by_kind(am.full_kwargs(kw), *ar.active_rows(A, l, u, e['x'], e['z'], e['y'], D, E, c)))
    return out


def _sets_of_single(name):
    kw, attrs, st, _ = _single(name)
    low, upp = ar.active_rows(st[1], st[2], st[3], *st[4:])
    return [bc.active_by_kind(am.full_kwargs(kw), low, upp)]


@pytest.mark.parametrize('name', bc.SINGLE)
def test_every_single_solve_is_solved_and_away_from_a_kink(name):
    kw, attrs, st, status = _single(name)
    assert status == 'solved', (name, status)
    l, u, z, y = st[2], st[3], st[5], st[6]
    # the golden fixtures are files: they are held to the device's own weak_tol (tests/adjoint_cases.STRICT); what this table makes itself
    # keeps the margin of tests/rollout_cases.py
    factor = 1.0 if name in bc.GOLDEN else rc.WEAK_FACTOR
    assert ar.count_weak(l, u, z, y, factor * WEAK_TOL) == 0, name
    print('BOUNDS_CASE %s: %s' % (name, _sets_of_single(name)[0]))


@pytest.mark.parametrize('key', list(bc.ROLLOUT) + list(bc.LOOPS), ids=str)
def test_every_loop_is_solved_and_away_from_a_kink(key):
    kw, attrs, tape, scaling = _tape(key)
    f = rc.tape_facts(kw, attrs, tape, scaling, weak_tol=WEAK_TOL)
    assert f['solved'].all(), (key, f['solved'])
    assert (f['n_weak'] == 0).all(), (key, f['n_weak'])              # (at rc.WEAK_FACTOR times weak_tol)
    print('BOUNDS_CASE %s: %s' % (key, _sets_of_tape(key)))


def _margin_entries():
    """The active sets, by kind, of every solve of the table that keeps the weak-row margin: (entry, SOFT_ON, sets)."""
    out = []
    for name in bc.SINGLE:
        kw, attrs, st, _ = _single(name)
        if ar.count_weak(st[2], st[3], st[5], st[6], rc.WEAK_FACTOR * WEAK_TOL) == 0:
            out.append((name, attrs.get('SOFT_ON', True), _sets_of_single(name)))
    for key in list(bc.ROLLOUT) + list(bc.LOOPS):
        out.append((key, _tape(key)[1].get('SOFT_ON', True), _sets_of_tape(key)))
    return out


def test_the_table_covers_the_rows():
    """Between the entries that keep the margin: the first Delta-u rows active on both sides, a state row active with slack columns and one
    without, state rows on both sides, input rows on both sides; the soft loop has five lower- and five upper-active state rows over its tape."""
    entries = _margin_entries()
    any_of = lambda kind, side, soft=None: any(s[kind][side] > 0 for _, so, sets in entries if soft is None or so == soft for s in sets)
    assert any_of('du_first', 0) and any_of('du_first', 1)
    assert any_of('state', 1, soft=True) and any_of('state', 0, soft=True)
    assert any_of('state', 0, soft=False) or any_of('state', 1, soft=False)
    assert any_of('input', 0) and any_of('input', 1) and any_of('du', 0) and any_of('du', 1)
    for key in bc.ROLLOUT:                                            # (what the existing loops do not reach: why LOOPS is there)
        assert all(s['state'] == (0, 0) and s['input'] == (0, 0) for s in _sets_of_tape(key)), key
    assert all(s['input'][0] > 0 and s['input'][1] > 0 for s in _sets_of_tape('ubox_tight'))
    soft = _sets_of_tape('xbox_soft')
    assert sum(s['state'][0] for s in soft) == 5 and sum(s['state'][1] for s in soft) == 5, soft
    assert all(s['state'][1] > 0 for s in _sets_of_tape('hard_state'))
    assert _sets_of_tape('cart_up')[0]['state'][1] > 0 and _sets_of_tape('cart_low')[0]['state'][0] > 0
    assert _sets_of_single(bc.HARD_STATE)[0]['state'][1] > 0 and bc.single(bc.HARD_STATE)[1] == {'SOFT_ON': False}


def test_every_bound_has_a_gradient_somewhere_and_infinite_bounds_have_none():
    rng = np.random.default_rng(5)
    seen = {n: 0.0 for n in br.NAMES}
    for name in bc.SINGLE:
        kw, attrs, st, _ = _single(name)
        if ar.count_weak(st[2], st[3], st[5], st[6], rc.WEAK_FACTOR * WEAK_TOL):
            continue
        r = ar.adjoint(*st, rng.standard_normal(st[0].shape[0]))
        for n, v in br.step(br.bound_maps(kw, attrs), r).items():
            seen[n] = max(seen[n], float(np.abs(v).max()))
    for key in list(bc.ROLLOUT[:3]) + list(bc.LOOPS):        # (the small ones)
        kw, attrs, tape, (D, E, c) = _tape(key)
        nx, nu = np.asarray(kw['Bd']).shape
        ref = br.sweep(kw, attrs, tape, D, E, c, rng.standard_normal((len(tape) + 1, nx)), rng.standard_normal((len(tape), nu)))
        for n in br.NAMES:
            seen[n] = max(seen[n], float(np.abs(ref[n]).max()))
    assert all(v > 1e-3 for v in seen.values()), seen
    # a bound that is infinite moves no row: zero columns, an exactly zero gradient
    from pympc_amd import fixtures
    kw = fixtures.quadcopter(finite_du=False)
    maps = br.bound_maps(kw)
    for n in ('Dumin', 'Dumax'):
        assert not maps[n][0].any() and not maps[n][1].any(), n
    inf_x = ~np.isfinite(kw['xmin'])
    assert inf_x.any() and not maps['xmin'][0][:, inf_x].any() and maps['xmin'][0][:, ~inf_x].any()
    assert not maps['xmin'][1].any() and not maps['xmax'][0].any()      # (a lower bound moves l alone, an upper one u alone)


def test_a_pair_of_equal_bounds_counts_in_the_lower_name():
    """umin = umax on one input: its rows are equalities, always active; d_l carries r_y and d_u nothing, so umin gets the derivative with
    respect to the common value and umax exactly 0."""
    kw, attrs = bc.loop('xbox_soft')
    kw = dict(kw, umin=np.array([-0.5, 0.1, -0.5]), umax=np.array([0.5, 0.1, 0.5]))
    import util
    K = util.oracle_controller(kw, attrs, eps=EPS, setup=True, quiet=True, max_iter=4000000)
    assert K.res.info.status == 'solved'
    x, z, y, _ = K.prob.iterate_state()
    D, E, c = K.prob.scaling()
    r = ar.adjoint(K.P, K.A, np.asarray(K.l, dtype=float), np.asarray(K.u, dtype=float), x, z, y, D, E, c, np.random.default_rng(1).standard_normal(K.P.shape[0]))
    g = br.step(br.bound_maps(kw, attrs), r)
    assert g['umax'][1] == 0.0 and abs(g['umin'][1]) > 1e-6, (g['umin'], g['umax'])


# ---- the restatement against central differences of the stepped loop ---------------------------------------------------------------------
def _loss(kw, attrs, K, Gx, Gu):
    _, X, U, _ = rc.oracle_rollout(kw, attrs, K, eps=EPS_FD)
    return float((Gx * X).sum() + (Gu * U).sum())


def test_the_restatement_against_central_differences():
    """L = sum_k <Gx[k], x_k> + sum_k <Gu[k], u_k> of the stepped loop on the oracle: bounds_ref.sweep against (L(b + h) - L(b - h)) / 2h in
    one entry of each of the six bounds -- the entry with the largest gradient -- on every loop of bounds_cases.FD_LOOPS, with H, EPS_FD and the acceptance of tests/test_rollout_cases.py: within 1e-4 max(1, |fd|_inf)."""
    checks, per_name = [], {n: 0.0 for n in br.NAMES}
    for key in bc.FD_LOOPS:
        kw, attrs, _, _ = _tape(key)
        kw = am.full_kwargs(kw)
        K = bc.LOOPS[key]['K']
        nx, nu = kw['Bd'].shape
        rng = np.random.default_rng(40)
        Gx, Gu = rng.standard_normal((K + 1, nx)), rng.standard_normal((K, nu))
        tape, X, U, (D, E, cs) = rc.oracle_rollout(kw, attrs, K, eps=EPS_FD)
        f = rc.tape_facts(kw, attrs, tape, (D, E, cs))
        assert f['solved'].all() and (f['n_weak'] == 0).all(), (key, f['solved'], f['n_weak'])
        for e in tape:                                               # (independent active rows: r_y is unique)
            (P, _, A, l, u), _ = am.build(rr.entry_kwargs(kw, e), attrs)
            act = np.flatnonzero(np.logical_or(*ar.active_rows(A, l, u, e['x'], e['z'], e['y'], D, E, cs)))
            assert np.linalg.matrix_rank(A[act]) == len(act), key
        ref = br.sweep(kw, attrs, tape, D, E, cs, Gx, Gu)
        assert ref['n_solved'] == K
        for n in br.NAMES:
            j = int(np.argmax(np.abs(ref[n])))
            vals = []
            for sgn in (1.0, -1.0):
                v = np.array(kw[n], dtype=float); v[j] += sgn * H
                vals.append(_loss(dict(kw, **{n: v}), attrs, K, Gx, Gu))
            checks.append(('%s %s[%d]' % (key, n, j), ref[n][j], (vals[0] - vals[1]) / (2 * H)))
            per_name[n] = max(per_name[n], abs(checks[-1][2]))
    scale = max(1.0, max(abs(v) for _, _, v in checks))
    for name, got, want in checks:
        print('BOUNDS_FD %s: ref %+.6e fd %+.6e' % (name, got, want))
    for name, got, want in checks:
        assert abs(got - want) <= 1e-4 * scale, (name, got, want)
    assert all(v > 1e-3 for v in per_name.values()), per_name         # (every kind of bound is held by a difference that is not in the noise)
