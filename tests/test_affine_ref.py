"""tests/affine_ref.py -- the CPU reference of the affine term x_{k+1} = Ad x_k + Bd u_k + d_k (l = u = -d_k on the dynamics rows of the oracle's
QP) -- pinned two independent ways before the GPU tests lean on it, and the condition of those tests checked on the oracle: every instance
ends 'solved' and has an active inequality row, so that the term reaches the projections.  Tight solves (eps 1e-9) held to 1e-6 relative, the
north-star tolerance of tests/test_gpu_backends.py.  No GPU needed."""
import warnings

import numpy as np
import pytest

import affine_ref as ar
import settings_cases as sc


def _controller(kw, attrs=None, eps=ar.TIGHT):
    from oracle.osqp_oracle import OSQP
    from pympc_amd import MPCController
    kw = dict(kw, eps_abs=eps, eps_rel=eps)
    K = MPCController(**kw)
    for a, v in (attrs or {}).items():
        setattr(K, a, v)
    K.prob = OSQP()
    K.solver_settings = dict(max_iter=200000)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        K.setup()
    assert K.res.info.status == 'solved'
    return K


def _close(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() <= 1e-6 * max(1e-3, np.abs(b).max())


@pytest.mark.parametrize('case', ['point_mass', 'quadcopter', 'cart_pole_nc1', 'random_12_4_30_hard', 'wide_25_8_3_tight'])
def test_a_constant_term_is_the_augmented_model(case):
    """[[Ad, d], [0, 1]] on the state [x; 1] with no weight and no bounds on the extra state: the same inputs and states.
    (Not on the cases whose soft state box is violated by O(1) under the term -- random_5_3_8, random_12_4_30_tight, group_3_2_50_20_tight: their
    slack cost eps_feas = 1e6 against weights of O(1) conditions the optimum so badly that two tight solves of two formulations of one problem
    agree to 1e-4 only, which says nothing about either.)"""
    kw, attrs = sc.draw(case)
    nx, nu, Np = ar.shape(case)
    d = ar.term(case, rows=1)[1, 0]
    K = ar.oracle(case, d)
    assert K.res.info.status == 'solved'
    aug = dict(kw)
    Ad, Bd = np.asarray(kw['Ad'], dtype=float), np.asarray(kw['Bd'], dtype=float).reshape(nx, -1)
    aug['Ad'] = np.block([[Ad, d[:, None]], [np.zeros((1, nx)), np.ones((1, 1))]])
    aug['Bd'] = np.vstack([Bd, np.zeros((1, nu))])
    aug['x0'] = np.append(np.asarray(kw['x0'], dtype=float), 1.0)
    pad = lambda M: np.block([[np.asarray(M, dtype=float), np.zeros((nx, 1))], [np.zeros((1, nx + 1))]])
    aug['Qx'] = pad(kw['Qx'])
    if 'QxN' in kw:
        aug['QxN'] = pad(kw['QxN'])
    xref = np.asarray(kw.get('xref', np.zeros(nx)), dtype=float)
    aug['xref'] = np.append(xref, 0.0) if xref.ndim == 1 else np.hstack([xref, np.zeros((xref.shape[0], 1))])
    for k, v in (('xmin', -np.inf), ('xmax', np.inf)):
        if k in kw:
            aug[k] = np.append(np.asarray(kw[k], dtype=float), v)
    Ka = _controller(aug, attrs)
    ou, oua = (Np + 1) * nx, (Np + 1) * (nx + 1)
    nU = K.Nc * nu
    assert _close(Ka.res.x[oua:oua + nU], K.res.x[ou:ou + nU])
    assert _close(Ka.res.x[:oua].reshape(Np + 1, nx + 1)[:, :nx], K.res.x[:ou].reshape(Np + 1, nx))


@pytest.mark.parametrize('case,rows', [('point_mass', None), ('quadcopter', 1), ('random_12_4_30_tight', None), ('random_12_4_30_tight', 1), ('group_3_2_50_20_tight', None)])
def test_without_active_bounds_the_term_is_a_shift_of_the_reference(case, rows):
    """Bounds wide enough to be inactive: the solution is the d-free problem's with the reference xref_k - xbar_k, shifted by the free response
    xbar_{k+1} = Ad xbar_k + d_k, xbar_0 = 0."""
    kw, attrs = sc.draw(case)
    nx, nu, Np = ar.shape(case)
    d = np.broadcast_to(ar.term(case, rows=rows)[2], (Np, nx))
    wide = dict(kw)
    for k in ('xmin', 'umin', 'Dumin'):
        wide[k] = -1e4 * np.ones_like(np.asarray(kw[k], dtype=float))
    for k in ('xmax', 'umax', 'Dumax'):
        wide[k] = 1e4 * np.ones_like(np.asarray(kw[k], dtype=float))
    K = _controller(wide, attrs)
    ar.put(K, d if rows is None else d[0])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        K.solve()
    assert K.res.info.status == 'solved'
    Ad = np.asarray(kw['Ad'], dtype=float)
    xbar = np.zeros((Np + 1, nx))
    for k in range(Np):
        xbar[k + 1] = Ad @ xbar[k] + d[k]
    xref = np.broadcast_to(np.asarray(kw.get('xref', np.zeros(nx)), dtype=float), (Np + 1, nx)) if np.ndim(kw.get('xref', np.zeros(nx))) == 1 \
        else np.asarray(kw['xref'], dtype=float)[:Np + 1]
    Ks = _controller(dict(wide, xref=xref - xbar), attrs)
    ou = (Np + 1) * nx
    nU = K.Nc * nu
    assert _close(K.res.x[ou:ou + nU], Ks.res.x[ou:ou + nU])
    assert _close(K.res.x[:ou].reshape(Np + 1, nx), Ks.res.x[:ou].reshape(Np + 1, nx) + xbar)
    assert np.abs(xbar).max() > 1e-3                      # (the shift is not nothing)


@pytest.mark.parametrize('case', sorted(ar.SCALE))
def test_every_instance_of_the_gpu_cases_is_solved_with_an_active_inequality(case):
    for rows in (None, 1) if case in ar.ONE_ROW else (None,):
        for x, y, status, l, u in ar.tight(case, rows):
            assert status == 'solved', (case, rows, status)
            assert ar.active_inequalities(case, x, l, u) >= 1, (case, rows)


@pytest.mark.parametrize('form', ar.FORMS)
def test_the_oracle_is_stable_on_the_loops_of_the_ill_conditioned_case(form):
    """random_12_4_30_tight at the x0 factors of affine_ref.LOOP_FACTORS: the oracle's two elimination orders (two roundings of one algorithm)
    take the same number of iterations in every solve of every instance's loop and end within 1e-8 of each other -- so a rounding-level
    difference on the device cannot move a stopping round, which on this case is worth 1e-6 of the trajectory."""
    case = 'random_12_4_30_tight'
    d0, dt, hold, mt = ar.schedule(case, form)
    w = sc.noise(ar.shape(case)[0])
    for b in range(ar.B):
        args = (case, b, sc.STEPS, w, None if d0 is None else d0[b], None if dt is None else dt[:, b], hold, None if mt is None else (mt[0][:, b], mt[1][:, b]), 2)
        ia, ic = [], []
        xa, ua, sa = ar.oracle_loop(*args, iters=ia)
        xc, uc, _ = ar.oracle_loop(*args, iters=ic, ordering=None)
        assert all(s == 'solved' for s in sa) and ia == ic, (form, b, ia, ic)
        assert np.abs(xa - xc).max() <= 1e-8 * max(1.0, np.abs(xa).max()) and np.abs(ua - uc).max() <= 1e-8 * max(1.0, np.abs(ua).max()), (form, b)


def test_the_polish_reference_is_exact_where_the_gpu_test_says_so():
    """random_12_4_30_tight: at affine_ref.POLISH_FACTORS the CPU restatement of OSQP's polish is accepted from the oracle's eps 1e-3 iterate on all
    three instances and gives the optimum (the tight solve, polished) to 1e-10, where the unpolished u0 is more than 1e-6 away; at factor 1.0 it is
    rejected on all three."""
    case = 'random_12_4_30_tight'
    opt, got = ar.polished(case, ar.TIGHT, ar.POLISH_FACTORS), ar.polished(case, sc.EPS, ar.POLISH_FACTORS)
    for (uo, so, _), (u, s, raw) in zip(opt, got):
        assert so == 1 and s == 1
        assert np.abs(u - uo).max() <= 1e-10 * max(1.0, np.abs(uo).max()) and np.abs(raw - uo).max() > 1e-6
    assert [s for _, s, _ in ar.polished(case, sc.EPS)] == [-1, -1, -1]
