"""The Riccati solver and its adjoint on the device (include/mpcqp_riccati.h, pympc_amd/csrc/mpcqp_riccati.h) against scipy and the numpy
restatement (tests/riccati_ref.py, pinned on the CPU by tests/test_riccati_ref.py) on its case list, three perturbed copies per case:
solution, both gain forms, residual, statuses and step counts; the adjoint against the restatement's and, on two small cases, against
central differences through the device's own forward; bit-identity of repeated calls, of batch positions and batch sizes, of host and
device pointers; mixed outcomes in one batch; the refusals; the torch layer.  The bounds are riccati_ref's: 100 x what the restatement itself
is away from scipy (floor 1e-13), 1e-5 against central differences.  Run with -s for the measured figures."""
import ctypes as C
import functools

import numpy as np
import pytest

import riccati_ref as rr

pytestmark = pytest.mark.gpu
NAMES = sorted(rr.CASES)
UNSTAB = (np.diag([1.2, 0.5]), np.array([[0.0], [1.0]]), np.eye(2), np.eye(1))      # an uncontrollable unstable mode


def _stack(insts):
    return tuple(np.stack([i[k] for i in insts]) for k in range(4))


@functools.lru_cache(maxsize=None)
def _ref(name):
    """Per copy: (scipy X, scipy K, scipy F, restatement of form 0, restatement of form 1); computed once, read-only afterwards."""
    out = []
    for A, B, Q, R in rr.copies(name):
        Xs, Ks = rr.scipy_dare(A, B, Q, R, 0)
        out.append((Xs, Ks, rr.scipy_dare(A, B, Q, R, 1)[1], rr.dare(A, B, Q, R, 0), rr.dare(A, B, Q, R, 1)))
    return out


@functools.lru_cache(maxsize=None)
def _dev(name, gf):
    from pympc_amd import riccati
    return riccati.dare(*_stack(rr.copies(name)), gain_form=gf)


# ---- 1. forward --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_solution_gains_and_residual(name):
    ref = _ref(name)
    fig = [0.0] * 6
    for gf in (0, 1):
        X, K, status, iters, res = _dev(name, gf)
        for b, (Xs, Ks, Fs, r0, r1) in enumerate(ref):
            r = r1 if gf else r0
            assert status[b] == 1 == r[2]
            assert abs(int(iters[b]) - r[3]) <= 1, (iters[b], r[3])
            assert np.array_equal(X[b], X[b].T)
            e = (rr.rel(X[b], Xs), rr.rel(K[b], Fs if gf else Ks), rr.rel(X[b], r[0]), rr.rel(K[b], r[1]))
            fig[0], fig[1 + gf], fig[3], fig[4], fig[5] = max(fig[0], e[0]), max(fig[1 + gf], e[1]), max(fig[3], e[2]), max(fig[4], e[3]), max(fig[5], res[b])
    print('RICCATI %-26s from scipy: X %.1e K %.1e F %.1e   from the restatement: X %.1e gain %.1e   res %.1e   steps %d'
          % (name, fig[0], fig[1], fig[2], fig[3], fig[4], fig[5], int(iters[0])))
    assert fig[0] <= rr.bound(name, 0) and fig[3] <= rr.bound(name, 0), (fig, rr.bound(name, 0))
    assert fig[1] <= rr.bound(name, 1) and fig[2] <= rr.bound(name, 2), (fig, rr.E_REF[name])
    assert fig[4] <= max(rr.bound(name, 1), rr.bound(name, 2))
    assert 0.0 <= fig[5] <= rr.res_bound(name), (fig[5], rr.res_bound(name))


def test_scalar_against_the_closed_form_root():
    a, b, q, r = (M[0, 0] for M in rr.SCALAR)
    X = _dev('scalar', 0)[0]
    root = rr.scalar_root(a, b, q, r)
    assert abs(X[0, 0, 0] - root) <= rr.FLOOR * root


def test_a_weight_that_is_not_positive_definite():
    from pympc_amd import riccati
    X, K, status, iters, res = riccati.dare(*_stack(rr.copies(rr.NOT_PD)))
    assert list(status) == [-1] * 3 and list(iters) == [0] * 3
    assert not X.any() and not K.any() and not res.any()


# ---- 2. adjoint --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', NAMES)
def test_adjoint_against_the_restatement(name):
    from pympc_amd import riccati
    insts = rr.copies(name)
    n, m = insts[0][1].shape
    G_X, G_K = rr.seeds(name, n, m)
    worst = 0.0
    for gf in (0, 1):
        X, K, status, _, _ = _dev(name, gf)
        g = riccati.dare_adjoint(*_stack(insts), X, K, status, G_X=G_X, G_K=G_K, gain_form=gf)
        for b, (A, B, Q, R) in enumerate(insts):
            r = _ref(name)[b][3 + gf]
            want = rr.dare_adjoint(A, B, Q, R, r[0], r[1], G_X, G_K, gf)
            for k, w in zip('ABQR', want[:4]):
                worst = max(worst, rr.rel(g[k][b], w))
            assert np.array_equal(g['Q'][b], g['Q'][b].T) and np.array_equal(g['R'][b], g['R'][b].T)
            assert abs(int(g['iters'][b]) - want[4]) <= 1
    print('RICCATI %-26s adjoint from the restatement: %.1e (bound %.1e)' % (name, worst, rr.adj_bound(name)))
    assert worst <= rr.adj_bound(name)


def _fd_device(forward, mats, symmetric, loss, h=1e-6):
    """Central differences of loss(forward(*mats)) in every entry of every matrix (symmetric directions where ``symmetric``; then the
    gradient of a symmetric perturbation), through the device: every perturbed problem is one instance of ONE batch."""
    pert, where = [], []
    for idx, M in enumerate(mats):
        for i in range(M.shape[0]):
            for j in range(i if symmetric[idx] else 0, M.shape[1]):
                E = np.zeros_like(M)
                E[i, j] = 1.0
                if symmetric[idx]:
                    E[j, i] = 1.0
                for s in (h, -h):
                    pert.append([a + s * E if k == idx else a for k, a in enumerate(mats)])
                where.append((idx, i, j))
    val = loss(*forward(*(np.stack([p[k] for p in pert]) for k in range(len(mats)))))
    grads = [np.zeros_like(M) for M in mats]
    for e, (idx, i, j) in enumerate(where):
        d = (val[2 * e] - val[2 * e + 1]) / (2 * h)
        if symmetric[idx] and i != j:
            grads[idx][i, j] = grads[idx][j, i] = d / 2
        else:
            grads[idx][i, j] = d
    return grads


@pytest.mark.parametrize('name', rr.SMALL_FD)
@pytest.mark.parametrize('gf', [0, 1])
def test_adjoint_against_central_differences_through_the_device(name, gf):
    from pympc_amd import riccati
    A, B, Q, R = rr.case(name)
    n, m = B.shape
    G_X, G_K = rr.seeds(name, n, m)
    X, K, status, _, _ = riccati.dare(A, B, Q, R, gain_form=gf)
    g = riccati.dare_adjoint(A, B, Q, R, X, K, status, G_X=G_X, G_K=G_K, gain_form=gf)
    fwd = lambda *M: riccati.dare(*M, gain_form=gf)[:2]
    fd = _fd_device(fwd, (A, B, Q, R), (False, False, True, True), lambda X, K: (G_X * X).sum(axis=(1, 2)) + (G_K * K).sum(axis=(1, 2)))
    for k, f in zip('ABQR', fd):
        e = rr.rel(g[k], f)
        print('RICCATI %s form %d d_%s against central differences of the device: %.1e' % (name, gf, k, e))
        assert e <= rr.FD_BOUND, (k, e)


# ---- 3. determinism and independence -----------------------------------------------------------------------------------------------------
def _mixed(names, count):
    """``count`` instances of one shape: perturbed copies of the named cases in turn, every seventh one not positive definite (R = 0)."""
    pools = [rr.copies(nm, 1 + (count + len(names) - 1) // len(names)) for nm in names]
    insts = [pools[i % len(names)][1 + i // len(names)] for i in range(count)]
    return [(A, B, Q, 0.0 * R) if i % 7 == 6 else (A, B, Q, R) for i, (A, B, Q, R) in enumerate(insts)]


@pytest.mark.parametrize('names', [('cart_pole', 'cart_pole_5ms'), ('random_17_3',)], ids=['4x1', '17x3'])
def test_bits_do_not_depend_on_the_call_the_position_or_the_batch_size(names):
    from pympc_amd import riccati
    insts = _mixed(names, 300)                     # more workgroups than the chip has compute units
    n, m = insts[0][1].shape
    G_X, G_K = rr.seeds('mixed', n, m)

    def run(sub):
        M = _stack(sub)
        fw = riccati.dare(*M)
        ad = riccati.dare_adjoint(*M, fw[0], fw[1], fw[2], G_X=G_X, G_K=G_K)
        return list(fw) + [ad[k] for k in ('A', 'B', 'Q', 'R', 'iters')]
    big, again = run(insts), run(insts)
    assert all(np.array_equal(a, b) for a, b in zip(big, again))
    assert sorted(set(big[2].tolist())) == [-1, 1] and np.all(np.isfinite(big[0])) and np.all(np.isfinite(big[5]))
    for pos in (0, 6, 149, 298):                   # alone, and as the last of three
        one, three = run(insts[pos:pos + 1]), run([insts[5], insts[200], insts[pos]])
        for full, a, b in zip(big, one, three):
            assert np.array_equal(full[pos], a[0]) and np.array_equal(full[pos], b[2]), pos


def test_mixed_outcomes_in_one_batch():
    """A converging instance between an unstabilizable one and one with R < 0: statuses (1, 0, -1) in place, zeros and no NaN where there is no
    solution, the converged instance's bits as if it were alone."""
    from pympc_amd import riccati
    good = rr.case('point_mass')
    neg = good[:3] + (-good[3],)
    order = [UNSTAB, good, neg, good]
    M = _stack(order)
    X, K, status, iters, res = riccati.dare(*M)
    assert status.tolist() == [0, 1, -1, 1]
    assert 1 <= iters[0] <= 50 and iters[2] == 0
    for out in (X, K, res):
        assert np.all(np.isfinite(out)) and not out[0].any() and not out[2].any()
    alone = riccati.dare(*good)
    for b in (1, 3):
        assert np.array_equal(X[b], alone[0]) and np.array_equal(K[b], alone[1]) and res[b] == alone[4] and iters[b] == alone[3]
    # under a budget that ends before the overflow, the budget is what ends the unstabilizable instance
    st8, it8 = riccati.dare(*M, max_iter=8)[2:4]
    assert st8.tolist() == [0, 0, -1, 0] and it8.tolist() == [8, 8, 0, 8]
    n, m = 2, 1
    G_X, G_K = rr.seeds('mixed', n, m)
    g = riccati.dare_adjoint(*M, X, K, status, G_X=G_X, G_K=G_K)
    ga = riccati.dare_adjoint(*good, alone[0], alone[1], alone[2], G_X=G_X, G_K=G_K)
    for k in 'ABQR':
        assert np.all(np.isfinite(g[k])) and not g[k][0].any() and not g[k][2].any()
        assert np.array_equal(g[k][1], ga[k]) and g[k][1].any()


def test_host_and_device_pointers_and_a_stream_of_ones_own():
    import torch
    from pympc_amd import riccati
    name = 'quadcopter'
    M = _stack(rr.copies(name))
    n, m = M[1].shape[1:]
    G_X, G_K = rr.seeds(name, n, m)
    host = _dev(name, 0)
    gh = riccati.dare_adjoint(*M, host[0], host[1], host[2], G_X=G_X, G_K=G_K)
    dev = torch.device('cuda:0')
    t = lambda a: torch.tensor(a, device=dev)
    Mt = [t(a) for a in M]
    same = lambda a, b: np.array_equal(a, b.cpu().numpy())
    for stream in (None, torch.cuda.Stream(device=dev)):
        with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
            out = riccati.dare(*Mt)
            gd = riccati.dare_adjoint(*Mt, out[0], out[1], out[2], G_X=t(G_X), G_K=t(G_K))
        if stream is not None:
            stream.synchronize()
        assert all(o.is_cuda for o in out)
        assert all(same(a, b) for a, b in zip(host, out))
        assert all(same(gh[k], gd[k]) for k in ('A', 'B', 'Q', 'R', 'iters'))


def test_sizes_beyond_the_limits_are_refused():
    from pympc_amd import _lib, riccati
    L = _lib.load()
    z, st = np.zeros(33 * 33), np.zeros(1, dtype=np.int32)
    p, ps = C.c_void_p(z.ctypes.data), C.c_void_p(st.ctypes.data)
    call = lambda n, m: L.mpcqp_dare(0, None, 1, n, m, None, p, p, p, p, p, p, ps, ps, p)
    assert call(33, 1) == -4 and call(1, 33) == -4 and call(0, 1) == -1      # MPCQP_ERR_UNSUPPORTED, MPCQP_ERR_ARG
    assert call(32, 32) == 0
    with pytest.raises(RuntimeError, match='not implemented'):
        riccati.dare(np.eye(33), np.ones((33, 1)), np.eye(33), np.eye(1))


def test_a_cross_term_and_the_two_designs():
    """S is folded in before the call (against scipy's s=); kalman_gain against pympc_amd.kalman.kalman_design_simple; lqr_terminal."""
    from pympc_amd import riccati, kalman
    import scipy.linalg as sla
    A, B, Q, R = rr.case('random_5_3')
    S = 0.1 * np.random.default_rng(3).standard_normal(B.shape)
    X, K, status, _, _ = riccati.dare(A, B, Q, R, S=S)
    Xs = sla.solve_discrete_are(A, B, Q, R, s=S)
    Ks = np.linalg.solve(R + B.T @ Xs @ B, B.T @ Xs @ A + S.T)
    assert status == 1 and rr.rel(X, Xs) <= rr.bound('random_5_3', 0) and rr.rel(K, Ks) <= rr.bound('random_5_3', 1)
    for nm in ('cart_pole', 'cart_pole_kalman'):
        Ad = rr._fixture(nm)[0]
        Cm = np.array([[1.0, 0, 0, 0], [0, 0, 1.0, 0]])
        Qn, Rn = np.diag([0.1, 10, 0.1, 10]) * 1e-2, 0.01 * np.eye(2)
        for kind in ('filter', 'predictor'):
            L, P, st = riccati.kalman_gain(Ad, Cm, Qn, Rn, type=kind)
            Lk, Pk, _ = kalman.kalman_design_simple(Ad, None, Cm, None, Qn, Rn, kind)
            case = 'kalman_dual_' + ('cart_pole' if nm == 'cart_pole' else 'cart_pole_5ms')
            assert st == 1 and L.shape == (4, 2), (nm, kind)
            assert rr.rel(P, Pk) <= rr.bound(case, 0) and rr.rel(L, Lk) <= rr.bound(case, 2 if kind == 'filter' else 1), (nm, kind)
    X, K = riccati.lqr_terminal(*rr.case('quadcopter'))
    assert rr.rel(X, _ref('quadcopter')[0][0]) <= rr.bound('quadcopter', 0)
    with pytest.raises(RuntimeError, match='without a solution'):
        riccati.lqr_terminal(*UNSTAB)


# ---- 4. torch ----------------------------------------------------------------------------------------------------------------------------
def _torch_case():
    import torch
    A, B, Q, R = rr.case('kalman_dual_cart_pole')          # (4, 2)
    G_X, G_K = rr.seeds('torch', 4, 2)
    dev = torch.device('cuda:0')
    return (A, B, Q, R), (G_X, G_K), dev, (lambda a, grad=False: torch.tensor(np.asarray(a, dtype=float), dtype=torch.float64, device=dev, requires_grad=grad))


@pytest.mark.parametrize('gf', [0, 1])
def test_torch_dare_against_central_differences(gf):
    from pympc_amd import riccati
    from pympc_amd.torch_layer import dare
    mats, (G_X, G_K), dev, t = _torch_case()
    P = [t(M, True) for M in mats]
    X, K = dare(*P, gain_form=gf)
    assert X.shape == (4, 4) and K.shape == (2, 4) and int(X.status) == 1
    ((t(G_X) * X).sum() + (t(G_K) * K).sum()).backward()
    fd = _fd_device(lambda *M: riccati.dare(*M, gain_form=gf)[:2], mats, (False, False, True, True),
                    lambda X, K: (G_X * X).sum(axis=(1, 2)) + (G_K * K).sum(axis=(1, 2)))
    for p, f, k in zip(P, fd, 'ABQR'):
        e = rr.rel(p.grad.cpu().numpy(), f)
        print('RICCATI torch dare form %d d_%s against central differences: %.1e' % (gf, k, e))
        assert e <= rr.FD_BOUND, (k, e)


@pytest.mark.parametrize('kind', ['filter', 'predictor'])
def test_torch_kalman_gain_against_central_differences(kind):
    from pympc_amd import riccati
    from pympc_amd.torch_layer import kalman_gain
    (At, Ct, Qn, Rn), (G_P, G_Lt), dev, t = _torch_case()
    mats = (At.T.copy(), Ct.T.copy(), Qn, Rn)              # A [4, 4], C [2, 4]
    G_L = G_Lt.T.copy()
    P = [t(M, True) for M in mats]
    L, Pm = kalman_gain(*P, type=kind)
    assert L.shape == (4, 2) and Pm.shape == (4, 4) and int(L.status) == 1
    ((t(G_L) * L).sum() + (t(G_P) * Pm).sum()).backward()
    fd = _fd_device(lambda *M: riccati.kalman_gain(*M, type=kind)[:2], mats, (False, False, True, True),
                    lambda L, Pm: (G_L * L).sum(axis=(1, 2)) + (G_P * Pm).sum(axis=(1, 2)))
    for p, f, k in zip(P, fd, ('A', 'C', 'Qn', 'Rn')):
        e = rr.rel(p.grad.cpu().numpy(), f)
        print('RICCATI torch kalman_gain %s d_%s against central differences: %.1e' % (kind, k, e))
        assert e <= rr.FD_BOUND, (k, e)


def test_torch_unbatched_parameters_get_the_batch_sum_and_failures_no_gradient():
    import torch
    from pympc_amd.torch_layer import dare
    insts = rr.copies('point_mass', 4)
    insts[2] = UNSTAB[:2] + insts[2][2:]                   # one instance without a solution
    A, B, Q, R = _stack(insts)
    G_X, G_K = rr.seeds('torch', 2, 1)
    dev = torch.device('cuda:0')
    t = lambda a, grad=False: torch.tensor(a, dtype=torch.float64, device=dev, requires_grad=grad)
    grads = []
    for batched in (True, False):
        Qt, Rt = (t(Q, True), t(R, True)) if batched else (t(Q[0], True), t(R[0], True))
        At, Bt = t(A, True), t(B, True)
        X, K = dare(At, Bt, Qt, Rt)
        assert X.status.tolist() == [1, 1, 0, 1] and not X[2].any()
        ((t(G_X) * X).sum() + (t(G_K) * K).sum()).backward()
        grads.append([p.grad.cpu().numpy() for p in (At, Bt, Qt, Rt)])
    per, shared = grads
    assert np.array_equal(per[0], shared[0]) and np.array_equal(per[1], shared[1])
    assert not per[0][2].any() and not per[2][2].any() and per[0][1].any()
    for k in (2, 3):
        assert shared[k].shape == per[k].shape[1:]
        assert np.abs(shared[k] - per[k].sum(axis=0)).max() <= 4 * 2.3e-16 * np.abs(per[k]).sum(axis=0).max()      # (two summation orders of four terms)


def test_a_terminal_weight_tied_to_the_model_backpropagates_through_both_paths():
    """u = mpc_step(K, x, u_prev, params = {Ad, QxN = dare(Ad, Bd, Qx, Qu)[0]}): the gradient of Ad is that of the dynamics rows plus that of
    the terminal weight through the Riccati equation; against a central difference of the same composition at small_mimo."""
    import torch
    import adjoint_model_ref as am
    from adjoint_cases import golden
    from util import repeated
    from pympc_amd import BatchMPCController, riccati
    from pympc_amd.torch_layer import mpc_step, dare
    B, eps, h = 2, 1e-11, 1e-5
    kw = am.full_kwargs(golden('small_mimo'))
    rng = np.random.default_rng(11)
    # (near the reference, from the reference input: with the cost-to-go as terminal weight the fixture's own x0 puts the first move on its
    #  rate bound, where u does not depend on the model at all)
    x = kw['xref'] + 0.3 * (np.stack([kw['x0']] * B) - kw['xref']) + 0.01 * rng.standard_normal((B, 2))
    um1 = np.stack([kw['uref']] * B) + 0.01 * rng.standard_normal((B, 2))
    w = rng.standard_normal((B, 2))
    dev = torch.device('cuda:0')
    t = lambda a, grad=False: torch.tensor(np.asarray(a, dtype=float), dtype=torch.float64, device=dev, requires_grad=grad)

    def controller():
        K = BatchMPCController(**repeated(kw, B, eps_feas=kw.get('eps_feas', 1e6), eps_abs=eps, eps_rel=eps, max_iter=400000))
        K.setup(solve=False)
        return K

    def u_of(Ad):
        K = controller()
        K.update_model(solve=False, Ad=np.stack([Ad] * B), QxN=np.stack([riccati.lqr_terminal(Ad, kw['Bd'], kw['Qx'], kw['Qu'])[0]] * B))
        return np.array(K.step(x, um1))
    Ad = t(kw['Ad'], True)
    QxN = dare(Ad, t(kw['Bd']), t(kw['Qx']), t(kw['Qu']))[0]
    K = controller()
    u = mpc_step(K, t(x), t(um1), params=dict(Ad=Ad, QxN=QxN))
    assert np.array_equal(u.detach().cpu().numpy(), u_of(kw['Ad']))
    (u * t(w)).sum().backward()
    grad = Ad.grad.cpu().numpy()
    direct = torch.autograd.grad((mpc_step(controller(), t(x), t(um1), params=dict(Ad=Ad, QxN=QxN.detach())) * t(w)).sum(), Ad)[0].cpu().numpy()
    fd = np.zeros((2, 2))
    for i in range(2):
        for j in range(2):
            E = np.zeros((2, 2))
            E[i, j] = h
            fd[i, j] = ((u_of(kw['Ad'] + E) - u_of(kw['Ad'] - E)) * w).sum() / (2 * h)
    print('RICCATI mpc_step(QxN = dare(Ad ..)) d_Ad against central differences: %.1e   share of the Riccati path: %.1e'
          % (rr.rel(grad, fd), rr.rel(direct, grad)))
    assert np.abs(fd).max() > 1e-1
    assert rr.rel(grad, fd) <= rr.FD_BOUND
    assert rr.rel(direct, grad) > 1e-3                      # (the path through QxN is part of it)
