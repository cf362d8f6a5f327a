"""The model gradients of the adjoint on the device (include/mpcqp_adjoint_model.h, pympc_amd/csrc/mpcqp_adjoint_model.h): the chain rule
alone against the header's sums on the device's own r_w, r_y and iterate; end to end against the numpy restatement
(tests/adjoint_model_ref.py, pinned on the CPU by tests/test_adjoint_model_reference.py) on the device's iterate; bit-identity with
mpcqp_adjoint, of a later solve and of repeated calls; the batch sum; statuses and errors; torch.autograd through mpc_step(params=...)
against central differences of the device solver; the example.  Settings and helpers are those of tests/test_gpu_adjoint.py (they live in
tests/adjoint_cases.py)."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest

import adjoint_cases as ac
import adjoint_ref as ar
import adjoint_model_ref as am
from adjoint_cases import (STRICT, TOL, EPS, RAW, CHAINED, golden, solved, device_state, random_batch, copies, snapshot, same, point_mass_batch,
                           case_batch)
from util import rel1_any

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODEL = am.NAMES
SHAPE_CASES = ['nb32_nu9_held', 'nb64_nu6', 'nb128_nu5', 'long200_nu2', 'nb32_np60', 'nb16_nu7_hard']


def _seed(bp):
    return np.random.default_rng(7).standard_normal((bp.batch, bp.n))


@functools.lru_cache(maxsize=None)
def _golden_case(name):
    """A strict fixture solved on the device and ONE call for q, l, u and the seven model gradients (computed once, read-only afterwards).
    'random_5_3_8_nc:xref2d': the fixture with its reference given row by row, rows that differ."""
    base, _, tag = name.partition(':')
    kw0 = golden(base)
    if tag:
        nx = np.asarray(kw0['Bd']).shape[0]
        kw0['xref'] = np.broadcast_to(kw0['xref'], (kw0['Np'] + 1, nx)) + 0.05 * np.random.default_rng(5).standard_normal((kw0['Np'] + 1, nx))
    K = solved(kw0)
    bp = K.prob.batch_problem
    g = _seed(bp)
    got = bp.adjoint(g_w=g, want=RAW + MODEL)
    info = bp.adjoint_info()
    kw = am.full_kwargs(kw0)
    data = dict(nx=bp.nx, nu=bp.nu, Np=bp.Np, Nc=bp.Nc, soft=kw0.attrs.get('SOFT_ON', True), xref=[kw['xref']], uref=[kw['uref']], uminus1=[kw['uminus1']])
    return bp, g, got, info, data, (kw, dict(kw0.attrs))


@functools.lru_cache(maxsize=None)
def _shape_case(name):
    K = case_batch(name)
    assert all(s == 'solved' for s in K.status()), (name, K.status())
    bp = K.prob
    g = _seed(bp)
    got = bp.adjoint(g_w=g, want=RAW + MODEL)
    info = bp.adjoint_info()
    c = ac.CASES[name]
    data = dict(nx=bp.nx, nu=bp.nu, Np=bp.Np, Nc=bp.Nc, soft=c['soft'], xref=np.asarray(K.xref), uref=np.asarray(K.uref), uminus1=np.asarray(K.uminus1))
    return bp, g, got, info, data, None


def _closed(data, b, w, y, r_w, r_y):
    return am.closed_form(data['nx'], data['nu'], data['Np'], data['Nc'], data['soft'], w, y, r_w, r_y, data['xref'][b], data['uref'][b], data['uminus1'][b])


# ---- 1. the chain alone ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', STRICT + ['random_5_3_8_nc:xref2d'] + SHAPE_CASES)
def test_the_chain_is_the_sums_of_the_header_on_the_devices_own_vectors(name):
    """The model outputs recomputed in numpy from the same call's -d_q = r_w, d_l + d_u = r_y, the iterate and the step data: within
    1e-12 of the sum of the absolute values of an entry's terms -- at most 2 (Np + 1) <= 402 of them bound the rounding of the two
    summation orders at 4.5e-14, this is twenty times that."""
    bp, g, got, (nact, nweak, status), data, _ = (_shape_case if name in ac.CASES else _golden_case)(name)
    x, _, y = bp.iterate_state()
    worst = 0.0
    for b in range(bp.batch):
        assert status[b] == 1, (name, b, status[b])
        cf, mag = _closed(data, b, x[b], y[b], -got['q'][b], got['l'][b] + got['u'][b])
        for k in MODEL:
            err, bound = np.abs(got[k][b] - cf[k]), 1e-12 * mag[k]
            assert np.all(err <= bound), (name, b, k, float(np.max(err)), float(np.max(bound)))
            worst = max(worst, float(np.max(err / np.maximum(mag[k], 1e-300))))
        for k in am.WEIGHTS:
            assert np.array_equal(got[k][b], got[k][b].T), (name, b, k)
        assert np.abs(got['Ad'][b]).max() > 0.0 and np.abs(got['Bd'][b]).max() > 0.0
        if not data['soft']:
            assert got['eps_feas'][b] == 0.0
    print('ADJOINT_MODEL_CHAIN %s: largest |device - numpy| / sum|terms| = %.3e' % (name, worst))


# ---- 2. end to end against the restatement on the device's iterate -----------------------------------------------------------------------
def _propagated_bound(data, b, w, y, r_w, r_y):
    """The bound of tests/test_gpu_adjoint.py on r_w, r_y -- TOL max(1, |.|_inf) each -- carried through the bilinear forms."""
    nx, nu, Np, Nc = data['nx'], data['nu'], data['Np'], data['Nc']
    N, n_x, n_u = Np + 1, (Np + 1) * nx, Nc * nu
    R, RYm = max(1.0, np.abs(r_w).max()), max(1.0, np.abs(r_y).max())
    X, U, Y = np.abs(w[:n_x]).reshape(N, nx), np.abs(w[n_x:n_x + n_u]).reshape(Nc, nu), np.abs(y[:n_x]).reshape(N, nx)
    XR = np.broadcast_to(np.asarray(data['xref'][b], dtype=float).reshape(-1, nx), (N, nx))
    dX = np.abs(w[:n_x].reshape(N, nx) - XR)
    Uv = w[n_x:n_x + n_u].reshape(Nc, nu)
    dUref = np.abs(Uv - data['uref'][b])
    dU = np.abs(Uv - np.vstack([data['uminus1'][b][None], Uv[:-1]]))
    iu = np.ones(Nc); iu[Nc - 1] = Np - Nc + 1
    two = np.full(Nc, 2.0); two[0] = 1.0                      # (RU_k - RU_{k-1} carries two errors, RU_0 one)
    pair = lambda v: 0.5 * (v[:, None] + v[None, :])          # sym of  e (x) v  with |e| <= 1 entrywise
    ku = np.minimum(np.arange(Np), Nc - 1)
    out = dict(Ad=TOL * (R * Y[1:].sum(0)[:, None] + RYm * X[:Np].sum(0)[None, :]),
               Bd=TOL * (R * Y[1:].sum(0)[:, None] + RYm * U[ku].sum(0)[None, :]),
               Qx=TOL * R * pair(dX[:Np].sum(0)), QxN=TOL * R * pair(dX[Np]),
               Qu=TOL * R * pair((iu[:, None] * dUref).sum(0)), QDu=TOL * R * pair((two[:, None] * dU).sum(0)),
               eps_feas=TOL * R * np.abs(w[n_x + n_u:]).sum() if data['soft'] else 0.0)
    return out


@pytest.mark.parametrize('name', STRICT + ['random_5_3_8_nc:xref2d'])
def test_model_gradients_are_the_restatement_on_the_devices_iterate(name):
    bp, g, got, (nact, nweak, status), data, (kw, attrs) = _golden_case(name)
    st = device_state(bp)
    ref = ar.adjoint(*st, g[0])
    assert status[0] == 1 and nweak[0] == 0 and ref['n_weak'] == 0 and nact[0] == ref['n_active'], name
    w, y = st[4], st[6]
    cf, _ = am.closed_form_of(kw, attrs, w, y, ref['r_w'], ref['r_y'])
    bound = _propagated_bound(data, 0, w, y, ref['r_w'], ref['r_y'])
    worst = {}
    for k in MODEL:
        err = np.abs(got[k][0] - cf[k])
        worst[k] = (float(np.max(err)), float(np.max(np.abs(cf[k]))), float(np.max(err / np.maximum(bound[k], 1e-300))))
    print('ADJOINT_MODEL_ERR %s: %s' % (name, '  '.join('%s err %.1e of %.1e (%.2g of the bound)' % ((k,) + v) for k, v in worst.items())))
    for k in MODEL:
        assert np.all(np.abs(got[k][0] - cf[k]) <= bound[k]), (name, k, worst[k])


# ---- 3. bit-identity ---------------------------------------------------------------------------------------------------------------------
def test_bit_identity_with_mpcqp_adjoint_of_a_later_solve_and_of_repeated_calls():
    from pympc_amd import fixtures
    kws = [fixtures.random_lti(i) for i in range(4)]
    Ka, Kb = (random_batch(kws, eps=1e-6) for _ in range(2))
    Ka.setup(); Kb.setup()
    before = snapshot(Ka.prob)
    assert same(before, snapshot(Kb.prob))
    g, gu = np.random.default_rng(3).standard_normal((4, Ka.prob.n)), np.ones((4, 4))
    plain = Kb.prob.adjoint(g_w=g, g_u0=gu, want=CHAINED + RAW)
    one = Ka.prob.adjoint(g_w=g, g_u0=gu, want=CHAINED + RAW + MODEL)
    assert np.all(Ka.prob.adjoint_info()[2] == 1)
    for k in CHAINED + RAW:
        assert np.array_equal(plain[k], one[k]), k
    only = Ka.prob.adjoint(g_w=g, g_u0=gu, want=MODEL)        # (no output of mpcqp_adjoint_io asked for)
    two = Ka.prob.adjoint(g_w=g, g_u0=gu, want=MODEL)
    s1 = Ka.prob.adjoint(g_w=g, g_u0=gu, want=MODEL, batch_sum=True)
    s2 = Ka.prob.adjoint(g_w=g, g_u0=gu, want=MODEL, batch_sum=True)
    for k in MODEL:
        assert np.array_equal(one[k], only[k]) and np.array_equal(one[k], two[k]) and np.array_equal(s1[k], s2[k]), k
        assert s1[k].shape == (1,) + one[k].shape[1:]
    assert same(before, snapshot(Ka.prob))
    x1 = np.stack([kw['x0'] for kw in kws]) * 0.9
    for K in (Ka, Kb):
        K.update(x1)
    assert same(snapshot(Ka.prob), snapshot(Kb.prob))
    ta, tb = Ka.run(3), Kb.run(3)
    for k in ('x', 'u', 'status', 'iter'):
        assert np.array_equal(ta[k], tb[k]), k


# ---- 4. the batch sum --------------------------------------------------------------------------------------------------------------------
def test_batch_sum_is_the_sum_over_the_batch():
    """37 instances (no multiple of the sum kernel's sixteen lanes): within B . 1.2e-16 . sum_b |term_b| . 4 of numpy's sum."""
    from pympc_amd import fixtures
    B = 37
    K = random_batch([fixtures.random_lti(i) for i in range(B)]); K.setup()
    assert all(s == 'solved' for s in K.status())
    g = np.random.default_rng(2).standard_normal((B, K.prob.n))
    per = K.prob.adjoint(g_w=g, want=MODEL)
    tot = K.prob.adjoint(g_w=g, want=MODEL, batch_sum=True)
    assert np.all(K.prob.adjoint_info()[2] == 1)
    for k in MODEL:
        err, bound = np.abs(tot[k][0] - per[k].sum(axis=0)), B * 1.2e-16 * 4 * np.abs(per[k]).sum(axis=0)
        assert np.all(err <= bound), (k, float(np.max(err)), float(np.max(bound)))
        assert np.abs(tot[k]).max() > 0.0


# ---- 5. statuses and errors --------------------------------------------------------------------------------------------------------------
def test_unsolved_instance_gets_zeros_and_adds_nothing_to_the_sum():
    name, bad = ac.INFEASIBLE
    s = ac.CASES[name]['seeds']
    Ka, Kb = case_batch(name, (s[0], s[1], bad, s[2])), case_batch(name, (s[0], s[1], s[2]))
    assert Ka.status() == ['solved', 'solved', 'primal infeasible', 'solved'], Ka.status()
    ga = np.random.default_rng(7).standard_normal((4, Ka.prob.n))
    ra, rb = Ka.prob.adjoint(g_w=ga, want=MODEL), Kb.prob.adjoint(g_w=ga[[0, 1, 3]], want=MODEL)
    assert list(Ka.prob.adjoint_info()[2]) == [1, 1, 0, 1]
    sa, sb = Ka.prob.adjoint(g_w=ga, want=MODEL, batch_sum=True), Kb.prob.adjoint(g_w=ga[[0, 1, 3]], want=MODEL, batch_sum=True)
    for k in MODEL:
        assert np.all(ra[k][2] == 0.0) and np.all(np.isfinite(ra[k])), k
        assert np.array_equal(ra[k][[0, 1, 3]], rb[k]), k
        bound = 4 * 1.2e-16 * 4 * np.abs(rb[k]).sum(axis=0)
        assert np.all(np.abs(sa[k] - sb[k]) <= bound), k
    assert all(np.any(rb['Ad'][b] != 0.0) for b in range(3))


def test_state_errors_carry_over():
    K, kw = point_mass_batch(um1_bad=[])
    K.setup(solve=False)
    gu = np.ones((K.B, K.nu))
    with pytest.raises(RuntimeError, match=r'\(-5\)'):          # MPCQP_ERR_STATE: nothing solved yet
        K.prob.adjoint(g_u0=gu, want=('Ad',))
    K.solve()
    assert np.any(K.adjoint(g_u0=gu, want=('Ad', 'Qx'))['Ad'] != 0.0)
    x, _, y = K.prob.iterate_state()
    for change in (lambda: K.update(K.x0, solve=False), lambda: K.update_model(Ad=K.Ad, solve=False), lambda: K.prob.warm_start(x, y)):
        change()
        with pytest.raises(RuntimeError, match='no solve since'):
            K.adjoint(g_u0=gu, want=('Bd',))
        with pytest.raises(RuntimeError, match='no solve since'):
            K.prob.adjoint(g_u0=gu, want=('x0', 'QDu'), batch_sum=True)
        K.solve()
        assert np.all(K.adjoint(g_u0=gu, want=MODEL)['status'] == 1)
    with pytest.raises(TypeError):
        K.prob.adjoint(g_u0=gu, want=('Cd',))


def test_raw_vector_mode_refuses_model_gradients():
    from pympc_amd.solver import DeviceProblem
    from polish_ref import golden_qp
    from util import load_golden
    P, q, A, l, u = golden_qp(load_golden('random_12_4_30_b'))
    prob = DeviceProblem()
    prob.setup(P, q, A, l, u, eps_abs=EPS, eps_rel=EPS, max_iter=400000)
    assert prob.solve().info.status == 'solved'
    bp = prob.batch_problem
    for k in MODEL:
        with pytest.raises(RuntimeError, match=r'\(-5\)'):
            bp.adjoint(g_u0=np.ones((1, bp.nu)), want=(k,))
    assert np.any(bp.adjoint(g_u0=np.ones((1, bp.nu)), want=RAW)['q'] != 0.0)      # the seam's own gradients as before


def test_struct_size_and_empty_requests_are_refused():
    from pympc_amd import _lib
    K = solved(golden('point_mass'))
    bp = K.prob.batch_problem
    gu, dst = np.ones((1, bp.nu)), np.zeros((1, bp.nx, bp.nx))
    io, mo = _lib.AdjointIO(), _lib.AdjointModelIO()
    io.struct_size, mo.struct_size = C.sizeof(_lib.AdjointIO), C.sizeof(_lib.AdjointModelIO)
    io.g_u0, mo.d_Ad = gu.ctypes.data, dst.ctypes.data
    call = lambda m: bp._L.mpcqp_adjoint_model(bp._h, C.byref(io), C.byref(m) if m is not None else None)
    assert call(mo) == 0 and np.any(dst != 0.0)
    mo.struct_size -= 8
    assert call(mo) == -1                                       # MPCQP_ERR_ARG
    mo.struct_size += 8
    mo.d_Ad = None
    assert call(mo) == -1                                       # nothing asked for
    io.struct_size += 8
    mo.d_Ad = dst.ctypes.data
    assert call(mo) == -1
    io.struct_size -= 8
    x0 = np.zeros((1, bp.nx))
    io.d_x0 = x0.ctypes.data
    assert call(None) == 0                                      # mo == NULL: mpcqp_adjoint
    assert np.array_equal(x0, bp.adjoint(g_u0=gu, want=('x0',))['x0'])


# ---- 6. torch: mpc_step(params=...) ------------------------------------------------------------------------------------------------------
PARAMS = ('Ad', 'Bd', 'Qx', 'QxN', 'Qu', 'QDu')


def _step_inputs(name, B):
    kw = am.full_kwargs(golden(name))
    nx, nu = kw['Bd'].shape
    rng = np.random.default_rng(11)
    x = np.stack([kw['x0']] * B) + 0.01 * rng.standard_normal((B, nx))
    um1 = np.stack([kw['uminus1']] * B) + 0.01 * rng.standard_normal((B, nu))
    w = rng.standard_normal((B, nu))
    return kw, x, um1, w


def _u_of(kw, B, x, um1, **model):
    """A fresh controller, the model put under it, one cold step: both ends of a difference alike (and what mpc_step's forward does)."""
    K = copies(kw, B); K.setup(solve=False)
    K.update_model(solve=False, **model)
    return np.array(K.step(x, um1))


@pytest.mark.parametrize('name', ['random_5_3_8_nc', 'small_mimo'])
def test_mpc_step_parameter_gradients_against_central_differences(name):
    """Every entry of the six matrices (a weight's (i, j) and (j, i) together), h = 1e-5, device solves at eps 1e-9 through update_model;
    bound 1e-4 max(1, |fd|_inf) as for the other gradients of the layer."""
    import torch
    from pympc_amd.torch_layer import mpc_step
    B = 3
    kw, x, um1, w = _step_inputs(name, B)
    dev = torch.device('cuda:0')
    base = {k: np.stack([kw[k]] * B) for k in PARAMS}
    params = {k: torch.tensor(v, dtype=torch.float64, device=dev, requires_grad=True) for k, v in base.items()}
    K = copies(kw, B); K.setup(solve=False)
    u = mpc_step(K, torch.tensor(x, device=dev), torch.tensor(um1, device=dev), params=params)
    assert np.array_equal(u.detach().cpu().numpy(), _u_of(kw, B, x, um1, **base))
    (u * torch.tensor(w, device=dev)).sum().backward()
    _, nweak, status = K.prob.adjoint_info()
    assert np.all(status == 1) and np.all(nweak == 0), (status, nweak)
    h = 1e-5
    for k in PARAMS:
        grad = params[k].grad
        assert grad is not None and tuple(grad.shape) == base[k].shape, k
        grad = grad.cpu().numpy()
        fd = np.zeros_like(base[k])
        for i, j in am._entries(k, base[k].shape[1:]):
            ends = []
            for s in (+h, -h):
                M = base[k].copy(); M[:, i, j] += s
                if k in am.WEIGHTS and i != j:
                    M[:, j, i] += s
                ends.append(_u_of(kw, B, x, um1, **dict(base, **{k: M})))
            v = ((ends[0] - ends[1]) * w).sum(axis=1) / (2 * h)      # (instances are independent: one batch perturbs all of them)
            if k in am.WEIGHTS and i != j:
                fd[:, i, j] = fd[:, j, i] = 0.5 * v
            else:
                fd[:, i, j] = v
        err, big = np.abs(grad - fd).max(), np.abs(fd).max()
        print('ADJOINT_MODEL_FD %s d/d%s: |grad - FD|_inf = %.3e, |FD|_inf = %.3e' % (name, k, err, big))
        assert err <= 1e-4 * max(1.0, big), (name, k, err)
        if k in ('Ad', 'Bd'):
            assert big > 1e-3, (name, k, big)


def test_mpc_step_unbatched_parameters_get_the_batch_sum_and_none_changes_nothing():
    import torch
    from pympc_amd.torch_layer import mpc_step
    B = 5
    kw, x, um1, w = _step_inputs('random_5_3_8_nc', B)
    dev = torch.device('cuda:0')
    tx, tu, tw = torch.tensor(x, device=dev), torch.tensor(um1, device=dev), torch.tensor(w, device=dev)
    grads = []
    for batched in (True, False):
        params = {k: torch.tensor(np.stack([kw[k]] * B) if batched else kw[k], dtype=torch.float64, device=dev, requires_grad=True) for k in ('Ad', 'Bd', 'Qx')}
        K = copies(kw, B); K.setup(solve=False)
        u = mpc_step(K, tx, tu, params=params)
        (u * tw).sum().backward()
        grads.append({k: p.grad.cpu().numpy() for k, p in params.items()})
    for k in ('Ad', 'Bd', 'Qx'):
        assert grads[1][k].shape == kw[k].shape, k
        bound = B * 1.2e-16 * 4 * np.abs(grads[0][k]).sum(axis=0)
        assert np.all(np.abs(grads[1][k] - grads[0][k].sum(axis=0)) <= bound), k
        assert np.abs(grads[1][k]).max() > 0.0
    # params=None: the layer as it was
    res = []
    for extra in ({}, dict(params=None)):
        K = copies(kw, B); K.setup(solve=False)
        t = tx.clone().requires_grad_(True)
        u = mpc_step(K, t, tu, **extra)
        (u * tw).sum().backward()
        res.append((u.detach().cpu().numpy(), t.grad.cpu().numpy()))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    with pytest.raises(TypeError):
        mpc_step(K, tx, tu, params=dict(xmin=tx))


def test_derivatives_after_a_step_are_those_of_the_u_prev_the_step_was_solved_with():
    """mpcqp_mpc_step leaves the applied input in the step data as the next u_{-1}; the active set of the first Delta-u rows and the QDu
    gradient belong to the one its solve was made with.  small_mimo sits on such a row: step() and update() + solve make the same solve, so
    gains, counts and model gradients after either agree (to the TOL of the other comparisons; the active sets exactly)."""
    B = 3
    kw, x, um1, w = _step_inputs('small_mimo', B)
    Ka, Kb = copies(kw, B), copies(kw, B)
    Ka.setup(solve=False); Kb.setup(solve=False)
    ua = np.array(Ka.step(x, um1))
    Kb.update(x, um1)
    assert np.abs(ua - Kb.prob.u0()).max() <= 1e-7 and all(s == 'solved' for s in Kb.status())
    Ga, Gb = Ka.gains(), Kb.gains()
    na, nb = Ka.prob.adjoint_info()[0], Kb.prob.adjoint_info()[0]
    N, nx, nu = kw['Np'] + 1, Ka.nx, Ka.nu
    assert np.array_equal(na, nb) and np.all(nb > N * nx), (na, nb)          # an inequality row is active ...
    ra, rb = (K.prob.adjoint(g_u0=w, want=('l', 'u') + MODEL) for K in (Ka, Kb))
    rdu = 2 * N * nx + Ka.Nc * nu
    assert np.all(np.any(rb['u'][:, rdu:rdu + nu] != 0.0, axis=1))             # ... among the first Delta-u rows, whose bounds carry u_{-1}
    for k in ('K_x0', 'K_um1', 'K_xref', 'K_uref'):
        assert rel1_any(Ga[k], Gb[k]) <= TOL, (k, rel1_any(Ga[k], Gb[k]))
    for k in ('l', 'u') + MODEL:      # (r_w, r_y depend on the active set alone; the model gradients also on the iterates, two solves at eps 1e-9)
        assert rel1_any(ra[k], rb[k]) <= (1e-6 if k in MODEL else TOL), (k, rel1_any(ra[k], rb[k]))
    assert np.array_equal(ra['l'] != 0.0, rb['l'] != 0.0) and np.array_equal(ra['u'] != 0.0, rb['u'] != 0.0)
    # the step data themselves still hold the applied input for the next step
    assert np.abs(np.array(Ka.step(x * 0.9)) - np.array(Kb.step(x * 0.9, ua))).max() <= 1e-7


def test_derivatives_after_a_device_loop_are_those_of_its_last_solve():
    """run() ends as the host loop does, with update(x, u) and a solve: the step data it leaves are the ones the iterate was solved with, so
    the calls after it agree with a twin stepped from the host."""
    B = 3
    kw, _, _, w = _step_inputs('small_mimo', B)
    Ka, Kb = copies(kw, B), copies(kw, B)
    Ka.setup(); Kb.setup()
    tr = Ka.run(2)
    x = np.stack([kw['x0']] * B)
    for _ in range(2):
        u = Kb.output()
        x = x @ kw['Ad'].T + u @ kw['Bd'].T
        Kb.update(x, u)
    assert np.abs(tr['x'][-1] - x).max() <= 1e-7 and all(s == 'solved' for s in Kb.status())
    Ga, Gb = Ka.gains(), Kb.gains()
    assert np.array_equal(Ka.prob.adjoint_info()[0], Kb.prob.adjoint_info()[0])
    for k in ('K_x0', 'K_um1', 'K_xref', 'K_uref'):
        assert rel1_any(Ga[k], Gb[k]) <= TOL, (k, rel1_any(Ga[k], Gb[k]))
    ra, rb = (K.prob.adjoint(g_u0=w, want=('l', 'u') + MODEL) for K in (Ka, Kb))
    assert np.array_equal(ra['l'] != 0.0, rb['l'] != 0.0) and np.array_equal(ra['u'] != 0.0, rb['u'] != 0.0)
    for k in MODEL:                       # (they carry the iterates of two solves at eps 1e-9 and u_{-1}: QDu would show a moved one)
        assert rel1_any(ra[k], rb[k]) <= 1e-6, (k, rel1_any(ra[k], rb[k]))
    assert np.abs(rb['QDu']).max() > 0.0


# ---- 7. the example ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_learn_model_example_descends():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'learn_model_through_mpc.py'), '--iters', '12'], capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-2000:]
    print(r.stdout)
    loss = [float(v) for v in re.findall(r'^iteration +\d+: loss ([0-9.e+-]+)', r.stdout, flags=re.M)]
    assert len(loss) == 13 and loss[-1] < loss[0], loss
    d = re.search(r'Ad ([0-9.e+-]+) -> ([0-9.e+-]+)', r.stdout)
    assert d and float(d.group(2)) < float(d.group(1)), r.stdout[-500:]
    active = re.search(r'expert: (\d+) of', r.stdout)
    assert active and int(active.group(1)) > 0                 # ... through a controller whose constraints are active
