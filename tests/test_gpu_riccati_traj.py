"""The Riccati difference equation and its adjoint on the device (include_ext3/mpcqp_riccati_traj.h, pympc_amd/csrc/mpcqp_riccati_traj.h)
against the CPU reference tests/riccati_traj_ref.py (pinned by tests/test_riccati_traj_ref.py) on its cases x steps x trajectory patterns:
trajectories, both gain forms, statuses, exact symmetry, host against device pointers; the adjoint against autograd through the reference for
seeds on X, on the gain and on both; repeated calls; a constant matrix against the sum over its trajectory form; the two outcomes that
end an instance early, beside untouched neighbours; the designs; the torch layer; the refusals; one closed loop end to end.  The bounds are
riccati_traj_ref's: 100 x the distance of the reference's two forms (floor 1e-13).  Run with -s for the measured figures."""
import ctypes as C
import functools

import numpy as np
import pytest

import riccati_ref as rr
import riccati_traj_ref as tr

pytestmark = pytest.mark.gpu
SEEDINGS = (('X', 0), ('K', 0), ('K', 1), ('XK', 0), ('XK', 1))      # (which outputs carry a seed, the gain form)
NAMES5 = ('A', 'B', 'Q', 'R', 'X0')


@functools.lru_cache(maxsize=None)
def _ref(name, T, pattern):
    return tr.run(tr.make(name, T, pattern), T)            # computed once, read-only afterwards


@functools.lru_cache(maxsize=None)
def _dev(name, T, pattern, gf):
    from pympc_amd import riccati
    m = tr.make(name, T, pattern)
    return riccati.dre(m['A'], m['B'], m['Q'], m['R'], m['X0'], gain_form=gf, T=T)


def _args(m):
    return tuple(m[k] for k in NAMES5)


# ---- 1. forward --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', tr.CASES)
def test_trajectories_and_both_gains(name):
    import torch
    from pympc_amd import riccati
    worst = 0.0
    for T in tr.STEPS:
        for pattern in tr.PATTERNS:
            m = tr.make(name, T, pattern)
            n, mm = m['B'].shape[-2:]
            Xr, Kr, Fr = _ref(name, T, pattern)
            for gf in (0, 1):
                X, K, status, bad = _dev(name, T, pattern, gf)
                assert X.shape == (T + 1, tr.BATCH, n, n) and K.shape == (T, tr.BATCH, mm, n)
                assert status.tolist() == [1] * tr.BATCH and bad.tolist() == [-1] * tr.BATCH
                assert np.array_equal(X, np.swapaxes(X, -1, -2))
                e = (tr.rel(X, Xr), tr.rel(K, Fr if gf else Kr))
                worst = max(worst, *e)
                assert max(e) <= tr.bound(name), (T, pattern, gf, e, tr.bound(name))
            dev = torch.device('cuda:0')
            out = riccati.dre(*(torch.tensor(a, device=dev) for a in _args(m)), gain_form=1, T=T)
            assert all(o.is_cuda for o in out)
            assert all(np.array_equal(a, b.cpu().numpy()) for a, b in zip(_dev(name, T, pattern, 1), out)), (T, pattern)
    print('RICCATI_TRAJ %-24s forward from the reference: %.1e (bound %.1e)' % (name, worst, tr.bound(name)))


def test_unbatched_inputs_and_a_held_matrix_with_T():
    from pympc_amd import riccati
    m = tr.make('random_5_3', 7, 'A')
    one = {k: (v[:, 0] if v.ndim == 4 else v[0]) for k, v in m.items()}
    X, K, status, bad = riccati.dre(*_args(one))           # [T, n, n] beside unbatched matrices: a trajectory
    assert X.shape == (8, 5, 5) and K.shape == (7, 3, 5) and int(status) == 1 and int(bad) == -1
    full = _dev('random_5_3', 7, 'A', 0)
    assert np.array_equal(X, full[0][:, 0]) and np.array_equal(K, full[1][:, 0])
    c = tr.make('random_5_3', 7, 'none')
    X, K, _, _ = riccati.dre(c['A'][0], c['B'][0], c['Q'][0], c['R'][0], c['X0'][0], T=7)
    assert np.array_equal(X, _dev('random_5_3', 7, 'none', 0)[0][:, 0])


# ---- 2. adjoint --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', tr.CASES)
def test_adjoint_against_autograd_through_the_reference(name):
    from pympc_amd import riccati
    worst, T = 0.0, 7
    for pattern in tr.PATTERNS:
        m = tr.make(name, T, pattern)
        G_X, G_K = tr.seeds(name, T, *m['B'].shape[-2:])
        for which, gf in SEEDINGS:
            gx, gk = (G_X if 'X' in which else None), (G_K if 'K' in which else None)
            X, _, status, _ = _dev(name, T, pattern, gf)
            g = riccati.dre_adjoint(*_args(m), X, status, G_X=gx, G_K=gk, gain_form=gf, T=T)
            again = riccati.dre_adjoint(*_args(m), X, status, G_X=gx, G_K=gk, gain_form=gf, T=T)
            want = tr.gradients(m, T, gx, gk, gf)
            for k in NAMES5:
                assert g[k].shape == m[k].shape and np.array_equal(g[k], again[k]), (pattern, which, gf, k)
                e = tr.rel(g[k], want[k])
                worst = max(worst, e)
                assert e <= tr.adj_bound(name), (pattern, which, gf, k, e, tr.adj_bound(name))
            for k in ('Q', 'R', 'X0'):
                assert np.array_equal(g[k], np.swapaxes(g[k], -1, -2)), k
    print('RICCATI_TRAJ %-24s adjoint from autograd through the reference: %.1e (bound %.1e)' % (name, worst, tr.adj_bound(name)))


@pytest.mark.parametrize('name', tr.CASES)
@pytest.mark.parametrize('T', [1, 2])
def test_adjoint_of_short_recursions(name, T):
    from pympc_amd import riccati
    m = tr.make(name, T, 'AB')
    G_X, G_K = tr.seeds(name, T, *m['B'].shape[-2:])
    for gf in (0, 1):
        X, _, status, _ = _dev(name, T, 'AB', gf)
        g = riccati.dre_adjoint(*_args(m), X, status, G_X=G_X, G_K=G_K, gain_form=gf)
        want = tr.gradients(m, T, G_X, G_K, gf)
        for k in NAMES5:
            assert tr.rel(g[k], want[k]) <= tr.adj_bound(name), (gf, k, tr.rel(g[k], want[k]))


@pytest.mark.parametrize('name', ['random_5_3', 'random_17_3'])
def test_a_constant_matrix_gets_the_sum_over_its_trajectory_form(name):
    from pympc_amd import riccati
    T = 7
    m = tr.make(name, T, 'none')
    G_X, G_K = tr.seeds(name, T, *m['B'].shape[-2:])
    rep = dict(m, A=np.stack([m['A']] * T), B=np.stack([m['B']] * T))
    X, _, status, _ = riccati.dre(*_args(m), T=T)
    Xr, _, _, _ = riccati.dre(*_args(rep))
    assert np.array_equal(X, Xr)
    held = riccati.dre_adjoint(*_args(m), X, status, G_X=G_X, G_K=G_K, T=T, want=('A', 'B'))
    per = riccati.dre_adjoint(*_args(rep), X, status, G_X=G_X, G_K=G_K, want=('A', 'B'))
    for k in 'AB':
        assert per[k].shape == (T,) + m[k].shape and held[k].shape == m[k].shape
        assert tr.rel(held[k], per[k].sum(axis=0)) <= tr.adj_bound(name), k


# ---- 3. outcomes that end an instance early ------------------------------------------------------------------------------------------------
def test_a_step_that_is_not_positive_definite_and_a_nan_beside_untouched_neighbours():
    from pympc_amd import riccati
    T = 7
    A, B, Q, R0 = rr.case(rr.NOT_PD)                       # cart_pole with Qu = 0: from X0 = 0, S_0 = 0
    good = rr.copies('cart_pole', 3)[1:]
    X0g = tr.initial('cart_pole', 4)
    rng = np.random.default_rng(2)
    At = np.stack([np.stack([A * (1 + 0.01 * rng.uniform(-1, 1, A.shape))] * 3) for _ in range(T)])
    mk = lambda rows: tuple(np.stack(r) for r in zip(*rows))
    Bm, Qm, Rm, X0 = mk([(B, Q, R0, 0.0 * X0g), (good[0][1], good[0][2], good[0][3], X0g), (good[1][1], good[1][2], good[1][3], X0g)])
    G_X, G_K = (g[:, :3] for g in tr.seeds('mixed', T, 4, 1))
    X, K, status, bad = riccati.dre(At, Bm, Qm, Rm, X0)
    assert status.tolist() == [-1, 1, 1] and bad.tolist() == [0, -1, -1]
    assert not X[:, 0].any() and not K[:, 0].any() and np.all(np.isfinite(X)) and X[:, 1].any()
    g = riccati.dre_adjoint(At, Bm, Qm, Rm, X0, X, status, G_X=G_X, G_K=G_K)
    two = riccati.dre(At[:, 1:], Bm[1:], Qm[1:], Rm[1:], X0[1:])
    g2 = riccati.dre_adjoint(At[:, 1:], Bm[1:], Qm[1:], Rm[1:], X0[1:], two[0], two[2], G_X=G_X[:, 1:], G_K=G_K[:, 1:])
    assert np.array_equal(X[:, 1:], two[0]) and np.array_equal(K[:, 1:], two[1])
    for k in NAMES5:
        batch = 1 if g[k].ndim == 4 else 0
        assert not np.take(g[k], 0, axis=batch).any() and np.all(np.isfinite(g[k])), k
        assert np.array_equal(np.take(g[k], [1, 2], axis=batch), g2[k]) and g2[k].any(), k
    # a NaN in one instance's A_traj[1]
    An = At.copy()
    An[1, 1, 2, 1] = np.nan
    Rg = np.stack([Rm[1]] * 3)
    Xn, Kn, status, bad = riccati.dre(An, np.stack([Bm[1]] * 3), np.stack([Qm[1]] * 3), Rg, np.stack([X0g] * 3))
    clean = riccati.dre(At, np.stack([Bm[1]] * 3), np.stack([Qm[1]] * 3), Rg, np.stack([X0g] * 3))
    assert status.tolist() == [1, 0, 1] and bad.tolist() == [-1, 1, -1]
    assert not Xn[:, 1].any() and not Kn[:, 1].any()
    for b in (0, 2):
        assert np.array_equal(Xn[:, b], clean[0][:, b]) and np.array_equal(Kn[:, b], clean[1][:, b])
    gn = riccati.dre_adjoint(An, np.stack([Bm[1]] * 3), np.stack([Qm[1]] * 3), Rg, np.stack([X0g] * 3), Xn, status, G_X=G_X, G_K=G_K)
    gc = riccati.dre_adjoint(At, np.stack([Bm[1]] * 3), np.stack([Qm[1]] * 3), Rg, np.stack([X0g] * 3), clean[0], clean[2], G_X=G_X, G_K=G_K)
    for k in NAMES5:
        batch = 1 if gn[k].ndim == 4 else 0
        assert not np.take(gn[k], 1, axis=batch).any(), k
        assert np.array_equal(np.take(gn[k], [0, 2], axis=batch), np.take(gc[k], [0, 2], axis=batch)), k


# ---- 4. the designs ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hold', [1, 3])
def test_kalman_gain_traj_and_lqr_traj_against_their_references(hold):
    from pympc_amd import riccati
    name = 'kalman_dual_cart_pole'
    A0, Ct, Qn, Rn = rr.case(name)
    rng = np.random.default_rng(40 + hold)
    A_traj = np.stack([np.stack([A0.T * (1 + 0.01 * rng.uniform(-1, 1, A0.shape)) for _ in range(2)]) for _ in range(4)])
    P0 = tr.initial(name, 4)
    L, P, status = riccati.kalman_gain_traj(A_traj, Ct.T.copy(), Qn, Rn, P0, hold=hold)
    Lr, Pr = tr.kalman_gain_traj(A_traj, Ct.T, Qn, Rn, P0, hold)
    assert L.shape == (4, 2, 4, 2) == Lr.shape and P.shape == (5, 2, 4, 4) == Pr.shape and status.tolist() == [1, 1]
    assert tr.rel(L, Lr) <= tr.bound(name) and tr.rel(P, Pr) <= tr.bound(name), (tr.rel(L, Lr), tr.rel(P, Pr))
    Lu, Pu, su = riccati.kalman_gain_traj(A_traj[:, 0], Ct.T.copy(), Qn, Rn, P0, hold=hold)      # unbatched
    assert Lu.shape == (4, 4, 2) and np.array_equal(Lu, L[:, 0]) and np.array_equal(Pu, P[:, 0]) and int(su) == 1
    # the cost-to-go of a schedule (each entry held `hold` steps by the caller: lqr_traj itself takes a model per step)
    name = 'random_5_3'
    A, B, Q, R = rr.case(name)
    Ad = np.repeat(np.stack([np.stack([A * (1 + 0.01 * rng.uniform(-1, 1, A.shape)) for _ in range(2)]) for _ in range(3)]), hold, axis=0)
    Bd = np.repeat(np.stack([np.stack([B * (1 + 0.01 * rng.uniform(-1, 1, B.shape)) for _ in range(2)]) for _ in range(3)]), hold, axis=0)
    QxN = tr.initial(name, 5)
    Pt, Kt = riccati.lqr_traj(Ad, Bd, Q, R, QxN)
    Ptr, Ktr = tr.lqr_traj(Ad, Bd, Q, R, QxN)
    assert Pt.shape == Ptr.shape == (3 * hold + 1, 2, 5, 5) and Kt.shape == Ktr.shape
    assert tr.rel(Pt, Ptr) <= tr.bound(name) and tr.rel(Kt, Ktr) <= tr.bound(name)
    with pytest.raises(RuntimeError, match='did not run through'):
        riccati.lqr_traj(Ad, Bd, Q, 0.0 * R, 0.0 * QxN)


# ---- 5. torch ----------------------------------------------------------------------------------------------------------------------------
def _t(dev):
    import torch
    return lambda a, grad=False: torch.tensor(np.asarray(a, dtype=float), dtype=torch.float64, device=dev, requires_grad=grad)


@pytest.mark.parametrize('gf', [0, 1])
@pytest.mark.parametrize('batched', [True, False], ids=['batched', 'unbatched-parameters'])
def test_torch_dre_against_the_reference_autograd(gf, batched):
    import torch
    from pympc_amd.torch_layer import dre
    name, T = 'random_5_3', 3
    m = tr.make(name, T, 'A')                              # A a trajectory, B one matrix
    if not batched:                                        # Q, R, X0 and B unbatched beside a batched trajectory: each gets the sum over the batch
        m = dict(m, B=m['B'][0], Q=m['Q'][0], R=m['R'][0], X0=m['X0'][0])
    full = {k: (v if v.ndim >= (4 if k == 'A' else 3) else np.stack([v] * tr.BATCH)) for k, v in m.items()}
    G_X, G_K = tr.seeds(name, T, 5, 3)
    t = _t(torch.device('cuda:0'))
    P = [t(m[k], True) for k in NAMES5]
    X, K = dre(*P, gain_form=gf)
    assert X.shape == (T + 1, tr.BATCH, 5, 5) and K.shape == (T, tr.BATCH, 3, 5) and X.status.tolist() == [1] * 3 and X.first_bad.tolist() == [-1] * 3
    ((t(G_X) * X).sum() + (t(G_K) * K).sum()).backward()
    want = tr.gradients(full, T, G_X, G_K, gf)
    for p, k in zip(P, NAMES5):
        w = want[k] if want[k].shape == tuple(p.shape) else want[k].sum(axis=0)
        assert tuple(p.grad.shape) == w.shape, k
        e = rr.rel(p.grad.cpu().numpy(), w)
        print('RICCATI_TRAJ torch dre form %d %s d_%s: %.1e' % (gf, 'batched' if batched else 'unbatched', k, e))
        assert e <= tr.adj_bound(name), (k, e)


@pytest.mark.parametrize('batched', [True, False], ids=['batched', 'unbatched-parameters'])
def test_torch_kalman_gain_traj_against_the_reference_autograd(batched):
    import torch
    from pympc_amd.torch_layer import kalman_gain_traj
    name, T, hold = 'random_5_3', 3, 2
    m = tr.make(name, T, 'A')
    A_traj, Cm = np.swapaxes(m['A'], -1, -2).copy(), np.swapaxes(m['B'], -1, -2).copy()
    Qn, Rn, P0 = m['Q'], m['R'], m['X0']
    if not batched:
        Cm, Qn, Rn, P0 = Cm[0], Qn[0], Rn[0], P0[0]
    rng = np.random.default_rng(8)
    G_L, G_P = rng.standard_normal((T, tr.BATCH, 5, 3)), rng.standard_normal((T + 1, tr.BATCH, 5, 5))
    G_P = 0.5 * (G_P + np.swapaxes(G_P, -1, -2))
    t = _t(torch.device('cuda:0'))
    P = [t(a, True) for a in (A_traj, Cm, Qn, Rn, P0)]
    L, Pt = kalman_gain_traj(*P, hold=hold)
    assert L.shape == (T, tr.BATCH, 5, 3) and Pt.shape == (T + 1, tr.BATCH, 5, 5) and L.status.tolist() == [1] * 3
    ((t(G_L) * L).sum() + (t(G_P) * Pt).sum()).backward()
    # the same on the CPU: the reference recursion on the dual problem, every entry held `hold` steps, seeds at the entries' first steps
    ct = lambda a: torch.tensor(a, dtype=torch.float64, requires_grad=True)
    Pc = [ct(a) for a in (A_traj, Cm, Qn, Rn, P0)]
    bc = lambda M: M if M.dim() == 3 else M.expand(tr.BATCH, *M.shape)
    with tr._one_thread():
        Xc, _, Fc = tr.recursion(Pc[0].transpose(-1, -2).repeat_interleave(hold, dim=0), bc(Pc[1]).transpose(-1, -2), bc(Pc[2]), bc(Pc[3]), bc(Pc[4]), T * hold)
        loss = (torch.tensor(G_L) * Fc[::hold].transpose(-1, -2)).sum() + (torch.tensor(G_P) * Xc[::hold]).sum()
        want = torch.autograd.grad(loss, Pc)
    assert rr.rel(L.detach().cpu().numpy(), Fc[::hold].transpose(-1, -2).detach().numpy()) <= tr.bound(name)
    for p, w, k in zip(P, want, ('A_traj', 'C', 'Qn', 'Rn', 'P0')):
        w = w.numpy()
        w = 0.5 * (w + np.swapaxes(w, -1, -2)) if k in ('Qn', 'Rn', 'P0') else w
        e = rr.rel(p.grad.cpu().numpy(), w)
        print('RICCATI_TRAJ torch kalman_gain_traj %s d_%s: %.1e' % ('batched' if batched else 'unbatched', k, e))
        assert tuple(p.grad.shape) == w.shape and e <= tr.adj_bound(name), (k, e)


def test_torch_instances_that_did_not_finish_contribute_no_gradient():
    import torch
    from pympc_amd.torch_layer import dre
    m = tr.make('random_5_3', 3, 'A')
    R = m['R'].copy()
    R[1] = -1e3 * R[1]                                     # S_0 = R + B'X0 B is negative definite
    t = _t(torch.device('cuda:0'))
    P = [t(a, True) for a in (m['A'], m['B'], m['Q'], R, m['X0'][0])]
    X, K = dre(*P)
    assert X.status.tolist() == [1, -1, 1] and X.first_bad.tolist() == [-1, 0, -1] and not X[:, 1].any()
    (X.sum() + K.sum()).backward()
    assert not P[0].grad[:, 1].any() and not P[3].grad[1].any() and P[0].grad[:, 0].any() and P[4].grad.any()


# ---- 6. the refusals -----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_anything_is_launched():
    from pympc_amd import _lib
    L = _lib.load()
    ARG, UNSUPPORTED = -1, -4
    z, st = np.zeros(8 * 33 * 33), np.zeros(1, dtype=np.int32)
    p, ps = C.c_void_p(z.ctypes.data), C.c_void_p(st.ctypes.data)
    st[0] = 7

    def dre(n=2, m=1, T=7, A_steps=7, B_steps=1, X0=p, s=None):
        return L.mpcqp_dre(0, None, 1, n, m, T, s, p, A_steps, p, B_steps, p, p, X0, p, p, ps, ps)

    def adj(n=2, m=1, T=7, A_steps=7, B_steps=1, G=p, d=p):
        return L.mpcqp_dre_adjoint(0, None, 1, n, m, T, None, p, A_steps, p, B_steps, p, p, p, p, None, G, G, d, d, d, d, d)
    for call in (dre, adj):
        assert call(n=33) == UNSUPPORTED and b'32' in L.mpcqp_last_error()
        assert call(m=33) == UNSUPPORTED
        assert call(T=0, A_steps=0) == ARG and call(n=0) == ARG
        assert call(A_steps=2) == ARG and b'A_steps' in L.mpcqp_last_error()
        assert call(B_steps=3) == ARG
    assert dre(X0=None) == ARG and b'must be given' in L.mpcqp_last_error()
    assert adj(G=None) == ARG and b'seed' in L.mpcqp_last_error()
    assert adj(d=None) == ARG
    s = _lib.RiccatiSettings()
    L.mpcqp_riccati_default_settings(C.byref(s))
    s.gain_form = 2
    assert dre(s=C.byref(s)) == ARG
    assert st[0] == 7 and not z.any()                      # nothing was launched: no output was written
    s.gain_form, s.max_iter, s.tol = 1, 0, -1.0            # (max_iter and tol are ignored)
    A, B, I2, R = np.stack([0.9 * np.eye(2)] * 7), np.ones((2, 1)), np.eye(2), np.eye(1)
    X, K, status, bad = np.zeros((8, 2, 2)), np.zeros((7, 1, 2)), np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
    q = lambda a: C.c_void_p(a.ctypes.data)
    assert L.mpcqp_dre(0, None, 1, 2, 1, 7, C.byref(s), q(A), 7, q(B), 1, q(I2), q(R), q(I2), q(X), q(K), q(status), q(bad)) == 0
    assert status[0] == 1 and bad[0] == -1 and np.array_equal(X[0], I2) and K.any()


# ---- 7. a closed loop end to end -------------------------------------------------------------------------------------------------------------
def test_a_noise_covariance_learns_through_the_time_varying_filter_and_the_loop():
    """rollout_tv_est on the cart pole (4, 1, 20), ny = 2, 6 steps, batch 2, with L_traj = kalman_gain_traj(..): the gradient of a trajectory
    loss with respect to Qn through torch_layer, against the same loop fed the CPU reference's gains and chained through its autograd.  The
    device gives d_L_traj in both."""
    import torch
    from util import repeated
    from pympc_amd import BatchMPCController, fixtures
    from pympc_amd.torch_layer import mpc_rollout_tv_est, kalman_gain_traj
    name, K, B = 'kalman_dual_cart_pole', 6, 2
    kw = fixtures.cart_pole()
    rng = np.random.default_rng(12)
    Adt = np.stack([np.stack([kw['Ad'] * (1 + 0.01 * rng.uniform(-1, 1, (4, 4))) for _ in range(B)]) for _ in range(K)])
    Cm = np.array([[1.0, 0, 0, 0], [0, 0, 1.0, 0]])
    Qn, Rn, P0 = np.diag([0.1, 10, 0.1, 10]) * 1e-2, 0.01 * np.eye(2), tr.initial(name, 4) * 0.01
    X0 = np.stack([[0.0, 0.0, 0.15 + 0.05 * b, 0.0] for b in range(B)])
    XH0 = X0 + 0.02 * rng.standard_normal(X0.shape)
    v, w = 0.005 * rng.standard_normal((K, B, 2)), 0.005 * rng.standard_normal((K, B, 4))
    t = _t(torch.device('cuda:0'))

    def ctrl():
        Kc = BatchMPCController(**repeated(kw, B, x0=XH0, eps_feas=kw.get('eps_feas', 1e6), eps_abs=1e-10, eps_rel=1e-10, max_iter=400000))
        Kc.setup(solve=False)
        return Kc

    def loss_of(L_traj):
        _, XH, _, U = mpc_rollout_tv_est(ctrl(), t(X0), t(XH0), K, t(Adt), None, 1, t(Cm), L_traj=L_traj, v=t(v), u_prev=t(np.zeros((B, 1))), w=t(w),
                                         params=dict(Ad=t(Adt[0])))
        return (U * U).sum() + (XH * XH).sum()
    tQ = t(Qn, True)
    L_dev, _ = kalman_gain_traj(t(Adt), t(Cm), tQ, t(Rn), t(P0))
    loss_of(L_dev).backward()
    # the reference's gains into the same loop; its d_L_traj chained through the reference's autograd
    cQ = torch.tensor(Qn, dtype=torch.float64, requires_grad=True)
    ct = lambda a: torch.tensor(np.broadcast_to(a, (B,) + a.shape).copy(), dtype=torch.float64)
    with tr._one_thread():
        _, _, Fc = tr.recursion(torch.tensor(np.swapaxes(Adt, -1, -2).copy()), ct(Cm.T), cQ.expand(B, 4, 4), ct(Rn), ct(P0), K)
    L_ref = Fc.transpose(-1, -2)
    assert rr.rel(L_dev.detach().cpu().numpy(), L_ref.detach().numpy()) <= tr.bound(name)
    L_in = t(L_ref.detach().numpy(), True)
    loss_of(L_in).backward()
    assert float(L_in.grad.abs().max()) > 0.0
    with tr._one_thread():
        want, = torch.autograd.grad((L_ref * L_in.grad.cpu()).sum(), [cQ])
    want = 0.5 * (want + want.T).numpy()
    e = rr.rel(tQ.grad.cpu().numpy(), want)
    print('RICCATI_TRAJ d loss / d Qn through the loop and the filter against the reference chain: %.1e (bound %.1e)' % (e, tr.adj_bound(name)))
    assert np.abs(want).max() > 0.0 and e <= tr.adj_bound(name), e
