"""The mathematics of the model gradients (include/mpcqp_adjoint_model.h), pinned on the CPU before any GPU is involved: the closed-form
sums of the header against gradients derived from the host builder by unit perturbation (tests/adjoint_model_ref.py), those against
central finite differences of the CPU oracle, and the symmetry and soft-constraint conventions.  tests/test_gpu_adjoint_model.py holds the
device to the same restatement.

FD_FIXTURES is fixed by name.  random_5_3_8 is not in it: its oracle solves carry about 1.7e-7 of path-dependent error in g'w, so its
finite-difference error scales as 1 / h (2.8e-3 at h = 1e-4, 1.7e-2 at 1e-5, 1.7e-1 at 1e-6) and says nothing about the gradient; it stays
in every comparison of the two restatements."""
import functools

import numpy as np
import pytest

import adjoint_ref as ar
import adjoint_model_ref as am
from adjoint_cases import STRICT, solve_golden, oracle_qp

FD_FIXTURES = ['random_5_3_8_nc', 'random_5_3_8_nc_hard', 'small_mimo', 'point_mass_nc', 'cart_pole_nc1', 'random_12_4_30_hard']


def _seed(kw, n, seed=3):
    """A random g_w on the x and u blocks (zero on the slack variables)."""
    nx, nu = kw['Bd'].shape
    Nc = kw['Np'] if kw.get('Nc') is None else kw['Nc']
    g = np.zeros(n)
    k = (kw['Np'] + 1) * nx + Nc * nu
    g[:k] = np.random.default_rng(seed).standard_normal(k)
    return g


@functools.lru_cache(maxsize=None)
def _case(name, xref2d=False):
    """The fixture solved by the oracle at eps 1e-11, the adjoint of a random seed on its iterate, and both restatements of the model
    gradients (computed once, read-only afterwards)."""
    kw0, (P, q, A, l, u), r, (x, z, y), (D, E, c) = solve_golden(name, 1e-11)
    kw, attrs = am.full_kwargs(kw0), dict(kw0.attrs)
    if xref2d:                                               # the same problem with its reference spelled out row by row, rows that differ
        nx = kw['Bd'].shape[0]
        kw['xref'] = np.broadcast_to(kw['xref'], (kw['Np'] + 1, nx)) + 0.05 * np.random.default_rng(5).standard_normal((kw['Np'] + 1, nx))
        (Pd, q, Ad_, l, u), K = am.build(kw, attrs)
        P, A = K.P, K.A
        o = oracle_qp(P, q, A, l, u, 1e-11)
        r = o.solve()
        assert r.info.status == 'solved'
        x, z, y, _ = o.iterate_state()
        D, E, c = o.scaling()
    g = _seed(kw, P.shape[0])
    res = ar.adjoint(P, A, l, u, x, z, y, D, E, c, g)
    grads, mags = am.builder_gradients(kw, attrs, x, y, res['r_w'], res['r_y'], res['low'], res['upp'])
    cf, cfm = am.closed_form_of(kw, attrs, x, y, res['r_w'], res['r_y'])
    return kw, attrs, g, (P, q, A, l, u), (x, y), res, grads, mags, cf, cfm


# ---- 1. the closed forms are what the builder implies --------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', STRICT + ['random_5_3_8:xref2d', 'random_12_4_30_hard:xref2d'])
def test_closed_forms_equal_the_builder_derived_gradients(name):
    """To 1e-12 of the sum of the absolute values of an entry's terms (rounding of at most 2 (Np + 1) products and of the unit differences
    of the builder's matrices), entry by entry, on every strict fixture and on references given row by row."""
    base, _, tag = name.partition(':')
    kw, attrs, g, qp, (x, y), res, grads, mags, cf, cfm = _case(base, bool(tag))
    for k in am.NAMES:
        bound = 1e-12 * np.maximum(mags[k], cfm[k])
        err = np.abs(grads[k] - cf[k])
        print('%s %s: |closed form - builder|_inf = %.3e, |gradient|_inf = %.3e' % (name, k, np.max(err), np.max(np.abs(cf[k]))))
        assert np.all(err <= bound), (name, k, float(np.max(err)), float(np.max(bound)))
    assert max(np.abs(cf[k]).max() for k in ('Ad', 'Bd', 'Qx')) > 0.0


# ---- 2. the restatement against central differences of the oracle --------------------------------------------------------------------------
@pytest.mark.parametrize('name', FD_FIXTURES)
def test_restatement_against_finite_differences(name):
    """L = g_w' w*(theta): every entry of Ad, Bd, of the weights (symmetric pairs) and eps_feas moved by h = 1e-5 either way, each end a cold
    solve of the oracle at eps 1e-11.  Bound 1e-4 max(1, |FD|_inf), as in tests/test_adjoint_reference.py."""
    kw, attrs, g, (P, q, A, l, u), (x, y), res, grads, mags, cf, cfm = _case(name)
    assert res['n_weak'] == 0
    h = 1e-5

    def loss(over):
        (_, q1, _, l1, u1), K = am.build(over, attrs)
        rr = oracle_qp(K.P, q1, K.A, l1, u1, 1e-11).solve()
        assert rr.info.status == 'solved'
        return float(g @ rr.x)

    for k in am.NAMES:
        if k == 'eps_feas':
            if not attrs.get('SOFT_ON', True):
                continue
            fd = np.float64((loss(am.perturbed(kw, k, 0, 0, h)) - loss(am.perturbed(kw, k, 0, 0, -h))) / (2 * h))
        else:
            fd = np.zeros(grads[k].shape)
            for i, j in am._entries(k, grads[k].shape):
                v = (loss(am.perturbed(kw, k, i, j, h)) - loss(am.perturbed(kw, k, i, j, -h))) / (2 * h)
                if k in am.WEIGHTS and i != j:
                    fd[i, j] = fd[j, i] = 0.5 * v            # (a pair moves both entries: dL = 2 d_Q[i, j])
                else:
                    fd[i, j] = v
        err, big = float(np.max(np.abs(grads[k] - fd))), float(np.max(np.abs(fd)))
        print('%s d_%s: |restatement - FD|_inf = %.3e, |FD|_inf = %.3e' % (name, k, err, big))
        assert err <= 1e-4 * max(1.0, big), (name, k, err, big)
        if k in ('Ad', 'Bd'):
            assert big > 1e-3, (name, k, big)                # ... of a gradient that is not zero


# ---- 3. conventions ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', STRICT)
def test_weight_gradients_are_symmetric_and_eps_feas_needs_slack_variables(name):
    kw, attrs, g, qp, (x, y), res, grads, mags, cf, cfm = _case(name)
    for G in (grads, cf):
        for k in am.WEIGHTS:
            assert np.array_equal(G[k], G[k].T), (name, k)
        if not attrs.get('SOFT_ON', True):
            assert G['eps_feas'] == 0.0, name
