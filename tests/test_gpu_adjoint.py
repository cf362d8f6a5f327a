"""Adjoint derivatives on the device (include/mpcqp_adjoint.h, pympc_amd/csrc/mpcqp_adjoint.h) against the numpy restatement
(tests/adjoint_ref.py) evaluated on the device's own iterate and scaling, on every KKT backend, on the headline shape against finite
differences of the device solver, without side effects on the handle, with the statuses it reports, against the unconstrained gains,
through torch.autograd and in the example.

Active sets are found at the project's parity setting eps_abs = eps_rel = 1e-9 unless a test says otherwise.  Values are compared on the
15 fixtures with strict complementarity (STRICT of tests/adjoint_cases.py, fixed by name); the six degenerate ones are only asked
to report n_weak > 0."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from util import load_golden, rel1_any, golden_backends
import adjoint_ref as ar
from adjoint_cases import (STRICT, EPS, TOL, RAW, CHAINED, golden, solved, device_state, random_batch, copies, snapshot, same,
                           point_mass_batch)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compare(bp, kw, label, b=0, maps=None):
    """mpcqp_adjoint with a random g_w (every output) and mpcqp_gains of instance b against the restatement on the device's own iterate.
    Returns (largest relative error, restatement of the seed)."""
    maps = ar.parameter_maps(kw, getattr(kw, 'attrs', {})) if maps is None else maps
    st = device_state(bp, b)
    g = np.random.default_rng(7).standard_normal((bp.batch, bp.n))
    ref = ar.adjoint(*st, g[b], maps)
    got = bp.adjoint(g_w=g, want=CHAINED + RAW)
    nact, nweak, status = bp.adjoint_info()
    assert status[b] == 1 and nweak[b] == 0 and ref['n_weak'] == 0, (label, status[b], nweak[b], ref['n_weak'])
    assert nact[b] == ref['n_active'], (label, nact[b], ref['n_active'])
    errs = {k: rel1_any(got[k][b], ref['d_' + k if k in RAW else k]) for k in CHAINED + RAW}
    assert np.all(got['l'][b][~ref['low']] == 0.0) and np.all(got['u'][b][~ref['upp']] == 0.0), label
    nu, nx = bp.nu, bp.nx
    Kref = ar.gains(*st, maps, (bp.Np + 1) * nx, nu)
    Kgot = bp.gains()
    nact2, nweak2, status2 = bp.adjoint_info()
    assert status2[b] == 1 and nweak2[b] == 0 and nact2[b] == Kref['n_active'], label
    for k, kk in (('x0', 'K_x0'), ('uminus1', 'K_um1'), ('xref', 'K_xref'), ('uref', 'K_uref')):
        errs[kk] = rel1_any(Kgot[k][b], Kref[kk])
    worst = max(errs.values())
    print('ADJOINT_ERR %s: max %.3e  %s' % (label, worst, ' '.join('%s=%.1e' % kv for kv in errs.items())))
    assert worst <= TOL, (label, errs)
    return worst, ref, got, Kgot


# ---- 1. every output against the restatement, on the strict fixtures ----------------------------------------------------------------------
@pytest.mark.parametrize('name', STRICT)
def test_adjoint_is_the_restatement(name):
    kw = golden(name)
    K = solved(kw)
    _compare(K.prob.batch_problem, kw, name)


# ---- 2. every backend --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', STRICT)
def test_adjoint_on_every_backend(name):
    """SOFT_ON = False (the *_hard fixtures), Nc < Np (*_nc, cart_pole_nc1) and a 2-D xref (point_mass_nc) are among the strict fixtures.
    The adjoint's own factor is generic: backends differ only through the iterate that fixes the active set."""
    from pympc_amd.solver import forced_settings
    kw = golden(name)
    maps = ar.parameter_maps(kw, kw.attrs)
    res = {}
    for be in golden_backends(name):
        with forced_settings(backend=be):
            K = solved(kw)
        bp = K.prob.batch_problem
        rhs = np.random.default_rng(0).standard_normal((1, bp.n))
        before = bp.kkt_solve(rhs)
        _, ref, got, Kgot = _compare(bp, kw, '%s-%s' % (name, be), maps=maps)
        assert np.array_equal(before, bp.kkt_solve(rhs)), be          # the handle's own factor is untouched
        res[be] = (ref, got, Kgot)
    base = res['sweeps']
    for be, (ref, got, Kgot) in res.items():
        assert np.array_equal(ref['low'], base[0]['low']) and np.array_equal(ref['upp'], base[0]['upp']), be
        for k in CHAINED + RAW:
            assert rel1_any(got[k], base[1][k]) <= TOL, (be, k, rel1_any(got[k], base[1][k]))
        for k in CHAINED:
            assert rel1_any(Kgot[k], base[2][k]) <= TOL, (be, k)


# ---- 3. the headline shape ---------------------------------------------------------------------------------------------------------------
def test_headline_batch_of_48():
    from pympc_amd import fixtures
    B = 48
    kws = [fixtures.random_lti(i) for i in range(B)]
    K = random_batch(kws); K.setup()
    assert all(s == 'solved' for s in K.status())
    bp = K.prob
    nx, nu, Np = 12, 4, 30
    refs = [ar.gains(*device_state(bp, b), ar.parameter_maps(kws[b]), (Np + 1) * nx, nu) for b in range(B)]
    G = K.gains()
    nact, nweak, status = bp.adjoint_info()
    assert np.all(status == 1) and np.all(nweak == 0) and np.all(G['n_weak'] == 0) and np.all(G['status'] == 1)
    worst = 0.0
    for b, ref in enumerate(refs):
        assert ref['n_weak'] == 0 and nact[b] == ref['n_active'], b
        for k in ('K_x0', 'K_um1', 'K_xref', 'K_uref'):
            worst = max(worst, rel1_any(G[k][b], ref[k]))
    nineq = [int(nact[b]) - (Np + 1) * nx for b in range(6)]
    print('ADJOINT_ERR headline48: max %.3e; active inequalities of the first six %s' % (worst, nineq))
    assert all(0 <= v <= 4 for v in nineq), nineq
    assert worst <= TOL, worst
    # finite differences of the device solver itself (eps 1e-9, h = 1e-5, cold solves at both ends) on four instances; tolerance as in the
    # CPU test: 1e-4 max(1, |J|_inf)
    h = 1e-5
    for b in (0, 1, 2, 5):
        pert = []
        for j in range(nx):
            for s in (+1.0, -1.0):
                kw = dict(kws[b]); x0 = np.array(kw['x0'], dtype=float); x0[j] += s * h; kw['x0'] = x0
                pert.append(kw)
        Kp = random_batch(pert); Kp.setup()
        assert all(s == 'solved' for s in Kp.status())
        u = Kp.prob.u0()
        J = np.stack([(u[2 * j] - u[2 * j + 1]) / (2 * h) for j in range(nx)], axis=1)
        err = np.abs(G['K_x0'][b] - J).max()
        print('ADJOINT_FD headline instance %d: |K_x0 - FD|_inf = %.3e, |J|_inf = %.3e' % (b, err, np.abs(J).max()))
        assert err <= 1e-4 * max(1.0, np.abs(J).max()), (b, err)


# ---- 4. no side effects ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('polish', [False, True])
def test_adjoint_and_gains_leave_the_handle_as_it_was(polish):
    from pympc_amd import fixtures
    kws = [fixtures.random_lti(i) for i in range(4)]
    Ka, Kb = (random_batch(kws, eps=1e-4, polish=polish) for _ in range(2))
    Ka.setup(); Kb.setup()
    before = snapshot(Ka.prob)
    assert same(before, snapshot(Kb.prob))
    g = np.random.default_rng(3).standard_normal((4, Ka.prob.n))
    Ka.prob.adjoint(g_w=g, g_u0=np.ones((4, 4)), want=CHAINED + RAW)
    Ka.gains()
    assert np.all(Ka.prob.adjoint_info()[2] == 1)
    assert same(before, snapshot(Ka.prob))
    # the next solve, and a 5-step device loop, against the twin that never took an adjoint
    x1 = np.stack([kw['x0'] for kw in kws]) * 0.9
    for K in (Ka, Kb):
        K.update(x1)
    assert same(snapshot(Ka.prob), snapshot(Kb.prob))
    Ka.gains()
    if polish:
        for K in (Ka, Kb):
            K.prob.update_settings(polish=False)             # (the device loop does not polish)
    ta, tb = Ka.run(5), Kb.run(5)
    for k in ('x', 'u', 'status', 'iter'):
        assert np.array_equal(ta[k], tb[k]), k
    assert same(snapshot(Ka.prob), snapshot(Kb.prob))


# ---- 5. statuses -------------------------------------------------------------------------------------------------------------------------
def test_infeasible_instance_reports_status_0_and_zero_outputs():
    K, _ = point_mass_batch()
    K.setup()
    assert K.status()[2] == 'primal infeasible'
    g = np.random.default_rng(1).standard_normal((5, K.prob.n))
    res = K.prob.adjoint(g_w=g, want=CHAINED + RAW)
    _, _, status = K.prob.adjoint_info()
    assert status[2] == 0 and all(status[b] == 1 for b in (0, 1, 3, 4)), status
    for k in CHAINED + RAW:
        assert np.all(res[k][2] == 0.0), k
        assert np.all(np.isfinite(res[k]))
    assert any(np.any(res[k][0] != 0.0) for k in RAW)
    G = K.gains()
    assert G['status'][2] == 0 and all(np.all(G[k][2] == 0.0) for k in ('K_x0', 'K_um1', 'K_xref', 'K_uref'))


def test_quadcopter_reports_weak_rows():
    K = solved(golden('quadcopter'))
    G = K.gains()
    assert G['status'] == 1 and G['n_weak'] > 0, G['n_weak']


def test_state_errors():
    K, _ = point_mass_batch()
    K.setup(solve=False)
    with pytest.raises(RuntimeError, match=r'\(-5\)'):          # MPCQP_ERR_STATE: nothing solved yet
        K.prob.adjoint(g_u0=np.ones((5, 1)))
    with pytest.raises(RuntimeError, match=r'\(-5\)'):
        K.prob.gains()
    with pytest.raises(ValueError):
        K.prob.adjoint()
    K.solve()
    K.prob.adjoint(g_u0=np.ones((5, 1)))
    assert np.all(K.prob.adjoint_info()[2][[0, 1, 3, 4]] == 1)


def test_raw_vector_mode_gives_the_seam_gradients_only():
    from pympc_amd.solver import DeviceProblem
    from polish_ref import golden_qp
    P, q, A, l, u = golden_qp(load_golden('random_12_4_30_b'))
    prob = DeviceProblem()
    prob.setup(P, q, A, l, u, eps_abs=EPS, eps_rel=EPS, max_iter=400000)
    assert prob.solve().info.status == 'solved'
    bp = prob.batch_problem
    for k in CHAINED:
        with pytest.raises(RuntimeError, match=r'\(-5\)'):
            bp.adjoint(g_u0=np.ones((1, bp.nu)), want=(k,))
    with pytest.raises(RuntimeError, match=r'\(-5\)'):
        bp.gains()
    g = np.random.default_rng(5).standard_normal((1, bp.n))
    ref = ar.adjoint(*device_state(bp), g[0])
    got = bp.adjoint(g_w=g, want=RAW)
    nact, nweak, status = bp.adjoint_info()
    assert status[0] == 1 and nweak[0] == 0 and nact[0] == ref['n_active']
    errs = {k: rel1_any(got[k][0], ref['d_' + k]) for k in RAW}
    print('ADJOINT_ERR csc_seam: %s' % errs)
    assert max(errs.values()) <= TOL, errs


def test_adjoint_settings_are_its_own():
    K = solved(golden('random_5_3_8'))
    bp = K.prob.batch_problem
    g = np.ones((1, bp.nu))
    a = bp.adjoint(g_u0=g)['x0'].copy()
    bp.update_settings(delta=1e-3, polish_refine_iter=0)       # the polish settings do not reach the adjoint
    assert np.array_equal(a, bp.adjoint(g_u0=g)['x0'])
    bp.set_adjoint(delta=1e-2, refine_iter=0)                  # its own do: one regularized solve, no refinement
    assert not np.array_equal(a, bp.adjoint(g_u0=g)['x0'])
    bp.set_adjoint(delta=1e-6, refine_iter=3)
    assert np.array_equal(a, bp.adjoint(g_u0=g)['x0'])
    with pytest.raises(RuntimeError, match=r'\(-1\)'):
        bp.set_adjoint(delta=0.0)


# ---- 6. the unconstrained gains ----------------------------------------------------------------------------------------------------------
def test_gains_without_active_inequalities_are_the_unconstrained_gains():
    from pympc_amd.unconstrained import unconstrained_gains
    kw = golden('random_12_4_30')
    K = solved(kw)
    G = K.gains()
    nx, nu = K.nx, K.nu
    assert G['status'] == 1 and G['n_weak'] == 0
    U = unconstrained_gains(kw['Ad'], kw['Bd'], kw['Np'], kw.get('Nc'), Qx=kw['Qx'], QxN=kw.get('QxN'), Qu=kw['Qu'], QDu=kw['QDu'])
    for k in ('K_x0', 'K_um1', 'K_xref', 'K_uref'):
        assert np.abs(G[k] - U[k][:nu]).max() <= 1e-8, (k, np.abs(G[k] - U[k][:nu]).max())


# ---- 7. torch ----------------------------------------------------------------------------------------------------------------------------
def test_mpc_step_gradients_against_central_differences():
    import torch
    from pympc_amd.torch_layer import mpc_step
    kw = dict(golden('random_5_3_8'))
    kw.setdefault('uminus1', np.array(kw['uref'], dtype=float))
    B, nx, nu = 8, 5, 3
    rng = np.random.default_rng(11)
    x = np.stack([kw['x0']] * B) + 0.01 * rng.standard_normal((B, nx))
    um1 = np.stack([kw['uminus1']] * B) + 0.01 * rng.standard_normal((B, nu))
    xref = np.stack([kw['xref']] * B) + 0.01 * rng.standard_normal((B, nx))
    w = rng.standard_normal((B, nu))

    def u_of(x_, um1_, xref_):                                   # a fresh controller, one cold step: both ends of a difference alike
        K = copies(kw, B); K.setup(solve=False)
        return np.array(K.step(x_, um1_, xref_))

    dev = torch.device('cuda:0')
    t = lambda a: torch.tensor(a, dtype=torch.float64, device=dev, requires_grad=True)
    tx, tu, tr = t(x), t(um1), t(xref)
    K = copies(kw, B); K.setup(solve=False)
    u = mpc_step(K, tx, tu, tr)
    assert u.shape == (B, nu) and u.requires_grad
    assert np.array_equal(u.detach().cpu().numpy(), u_of(x, um1, xref))
    (u * torch.tensor(w, device=dev)).sum().backward()
    _, nweak, status = K.prob.adjoint_info()
    assert np.all(status == 1) and np.all(nweak == 0), (status, nweak)
    h = 1e-5
    for name, base, grad in (('x', x, tx.grad), ('u_prev', um1, tu.grad), ('xref', xref, tr.grad)):
        assert grad is not None and grad.shape == base.shape, name
        fd = np.zeros_like(base)
        for j in range(base.shape[1]):
            args = dict(x=x, u_prev=um1, xref=xref)
            up, dn = base.copy(), base.copy()
            up[:, j] += h; dn[:, j] -= h
            args[name] = up; a = u_of(args['x'], args['u_prev'], args['xref'])
            args[name] = dn; b = u_of(args['x'], args['u_prev'], args['xref'])
            fd[:, j] = ((a - b) * w).sum(axis=1) / (2 * h)       # (instances are independent: one batch perturbs all eight)
        err = np.abs(grad.cpu().numpy() - fd).max()
        print('ADJOINT_FD torch d/d%s: |grad - FD|_inf = %.3e, |FD|_inf = %.3e' % (name, err, np.abs(fd).max()))
        assert err <= 1e-4 * max(1.0, np.abs(fd).max()), (name, err)
        if name == 'x':                                          # (at this point the law hardly depends on u_prev and xref: the restatement's
            assert np.abs(fd).max() > 1e-3                       #  K_um1 and K_xref are below 1e-6 -- their gradients are checked as values)


def test_mpc_step_failed_instances_get_zero_gradients_and_a_second_step_is_refused():
    import torch
    from pympc_amd.torch_layer import mpc_step
    K, kw = point_mass_batch()
    K.setup(solve=False)
    dev = torch.device('cuda:0')
    t = lambda a: torch.tensor(np.asarray(a, dtype=float), dtype=torch.float64, device=dev, requires_grad=True)
    tx, tu, tr = t(K.x0), t(K.uminus1), t(K.xref)
    u = mpc_step(K, tx, tu, tr)
    assert K.status()[2] == 'primal infeasible'
    assert np.array_equal(u.detach().cpu().numpy()[2], np.asarray(kw['uref'], dtype=float))      # u_failure
    u.sum().backward()
    for g in (tx.grad, tu.grad, tr.grad):
        assert torch.all(g[2] == 0) and torch.all(torch.isfinite(g))
    # the solved instances sit on the first Delta-u row's bound, u_0 = u_prev + Dumax: the gradient reaches u_prev (K_um1 = 1 in the restatement)
    assert torch.any(tu.grad[[0, 1, 3, 4]] != 0)
    # the controller moves on between forward and backward: the backward refuses
    u = mpc_step(K, tx, tu, tr)
    K.step(K.x0, K.uminus1, K.xref)
    with pytest.raises(RuntimeError, match='stepped or solved again'):
        u.sum().backward()


def test_adjoint_waits_for_a_solve_after_anything_that_replaces_its_inputs():
    """Step data, model or iterate replaced without a solve: the iterate no longer belongs to what k_adjoint would read beside it, so the
    calls refuse (MPCQP_ERR_STATE) until the next solve -- also through mpc_step's backward."""
    import torch
    from pympc_amd.torch_layer import mpc_step
    K, kw = point_mass_batch(um1_bad=[])
    K.setup()
    ref = K.gains()
    assert np.all(ref['status'] == 1)
    x, _, y = K.prob.iterate_state()
    for change in (lambda: K.update(K.x0, solve=False), lambda: K.update_model(Ad=K.Ad, solve=False), lambda: K.prob.warm_start(x, y)):
        change()
        with pytest.raises(RuntimeError, match='no solve since'):
            K.gains()
        with pytest.raises(RuntimeError, match='no solve since'):
            K.adjoint(g_u0=np.ones((K.B, K.nu)))
        K.solve()
        assert np.all(K.gains()['status'] == 1)
    dev = torch.device('cuda:0')
    t = lambda a: torch.tensor(np.asarray(a, dtype=float), dtype=torch.float64, device=dev, requires_grad=True)
    tx = t(K.x0)
    u = mpc_step(K, tx, t(K.uminus1), t(K.xref))
    K.update(K.x0, solve=False)                     # (no solve: the layer's own count of solves does not see it, the library does)
    with pytest.raises(RuntimeError, match='no solve since'):
        u.sum().backward()


def test_adjoint_out_buffers_are_checked():
    K, kw = point_mass_batch(um1_bad=[])
    K.setup()
    g = np.ones((K.B, K.nu))
    with pytest.raises(ValueError, match='out'):
        K.prob.adjoint(g_u0=g, want=('x0',), out=dict(x0=np.empty((K.B, K.nx - 1))))
    with pytest.raises(ValueError, match='out'):
        K.prob.adjoint(g_u0=g, want=('x0',), out=dict(x0=np.empty((K.B, K.nx), dtype=np.float32)))
    ok = np.empty((K.B, K.nx))
    assert K.prob.adjoint(g_u0=g, want=('x0',), out=dict(x0=ok))['x0'] is ok


def test_mpc_step_gradient_reaches_a_reference_the_law_depends_on():
    """On headline instance 2 (four inequalities active at the optimum) the law depends on the reference at order one: the xref gradient
    through mpc_step, for a one-row and for an (Np+1)-row reference, against central differences of step() along random directions."""
    import torch
    from pympc_amd import fixtures
    from pympc_amd.torch_layer import mpc_step
    kw = dict(fixtures.random_lti(2)); kw['Np'] = 30
    B, nx, nu, N = 3, 12, 4, 31
    rng = np.random.default_rng(5)
    x = np.stack([kw['x0']] * B) * (1.0 + 0.01 * rng.standard_normal((B, 1)))
    um1 = np.stack([kw['uminus1']] * B)
    w = rng.standard_normal((B, nu))
    dev = torch.device('cuda:0')

    def u_of(xref_):
        K = copies(kw, B); K.setup(solve=False)
        return np.array(K.step(x, um1, xref_.reshape(B, -1)))

    for rows in (1, N):
        shape = (B, nx) if rows == 1 else (B, N, nx)
        xref = np.broadcast_to(np.asarray(kw['xref'], dtype=float), shape) + 0.01 * rng.standard_normal(shape)
        tr = torch.tensor(xref, dtype=torch.float64, device=dev, requires_grad=True)
        K = copies(kw, B); K.setup(solve=False)
        u = mpc_step(K, torch.tensor(x, device=dev), torch.tensor(um1, device=dev), tr)
        (u * torch.tensor(w, device=dev)).sum().backward()
        _, nweak, status = K.prob.adjoint_info()
        assert np.all(status == 1) and np.all(nweak == 0), (status, nweak)
        assert tr.grad.shape == shape
        g = tr.grad.cpu().numpy()
        h, big = 1e-5, 0.0
        for _ in range(3):
            d = rng.standard_normal(shape)
            d /= np.sqrt((d * d).sum(axis=tuple(range(1, d.ndim)), keepdims=True))      # a unit direction per instance
            fd = ((u_of(xref + h * d) - u_of(xref - h * d)) * w).sum(axis=1) / (2 * h)
            an = (g * d).reshape(B, -1).sum(axis=1)
            err = np.abs(an - fd).max()
            print('ADJOINT_FD torch d/dxref (%d rows): |grad.d - FD|_inf = %.3e, |FD|_inf = %.3e' % (rows, err, np.abs(fd).max()))
            assert err <= 1e-4 * max(1.0, np.abs(fd).max()), (rows, err)      # (the bound of the central differences above)
            big = max(big, np.abs(fd).max())
        assert big > 1e-2, big                                                 # ... of a gradient that is not zero


# ---- 8. the example ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.timeout(300)
def test_differentiable_mpc_example_descends():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'differentiable_mpc.py')], capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-2000:]
    print(r.stdout)
    loss = [float(v) for v in re.findall(r'^iteration +\d+: loss ([0-9.e+-]+)', r.stdout, flags=re.M)]
    assert len(loss) >= 11, r.stdout
    assert all(b < a for a, b in zip(loss[:10], loss[1:11])), loss[:11]
    # ... and it falls BY WHAT THE GRADIENT SAYS: the example accepts a step only at a quarter of the first-order prediction step |grad|^2
    # (its Armijo rule), and on a piecewise quadratic loss a correct gradient gives 1 - O(step), never much above 1 -- a gradient that is
    # too small by a factor, or a direction that is merely downhill, fails one side or the other.  The default step needs no halving: the
    # loss is a mean of squares of states that move O(1) with xref through a plant of spectral radius below 1, curvature of order 1 against
    # a step of 0.1; two halvings are allowed for, more would mean the gradient is not one.
    ratio = [float(v) for v in re.findall(r'decrease / predicted ([0-9.e+-]+)', r.stdout)][:10]      # (the first line, before any step, prints nan)
    halvings = [int(v) for v in re.findall(r'halvings (\d+)', r.stdout)]
    assert len(ratio) == 10 and all(0.25 <= v <= 1.25 for v in ratio), ratio
    assert halvings[10] <= 2, halvings
