"""mpcqp_update_model / mpcqp_mpc_loop_tv (include/mpcqp_model.h) on the device.

The contract is bit-identity with the route a caller had before: mpcqp_get_iterate, mpcqp_setup with the merged model and the same step data
(or raw vectors), mpcqp_warm_start(x, y), mpcqp_solve -- for every KKT backend a fixture is eligible for (tests/test_gpu_backends.py decides), on
single controllers, batches, shared factors, the follow-on paths (mpcqp_step_host, polishing) and the device loop; plus the oracle's answers
(fresh setup + warm start from the same iterate) at the tolerances of tests/test_gpu_parity.py."""
import contextlib
import ctypes as C
import warnings

import numpy as np
import pytest
import scipy.sparse as sp

from util import load_golden, golden_kwargs, controller, rel, stacked_batch, forced, golden_backends
from ltv_models import new_model, with_model, model_schedule

pytestmark = pytest.mark.gpu

NAMES = ['cart_pole', 'quadcopter_nc', 'random_12_4_30', 'random_20_8_12_hard', 'point_mass']
CASES = [(n, t) for n in NAMES for t in golden_backends(n)]
IDS = ['%s-%s' % c for c in CASES]
ERR_ARG, ERR_UNSUPPORTED, ERR_STATE, NON_CVX = -1, -4, -5, -7


def _info(i):
    return (i.status, i.iter, i.rho_updates, i.obj_val, i.pri_res, i.dua_res, i.rho)


def _res_info(r):
    i = r.info
    return (i.status_val, i.iter, i.rho_updates, i.obj_val, i.pri_res, i.dua_res, i.rho_estimate)


@contextlib.contextmanager
def _quiet():
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        yield


def test_cases_cover_every_backend():
    assert {t for _, t in CASES} == {'sweeps', 'dense', 'bcr', 'bcr8', 'bcrt'} and {n for n, _ in CASES} == set(NAMES)


@pytest.mark.parametrize('name,tag', CASES, ids=IDS)
def test_qp_scaling_and_iterate_after_update_model(name, tag):
    """export_qp: P, A bit-exact against qp_build for the new model, q to rtol 2e-15 (the bound of test_device_built_qp_matches_reference);
    D, E, c, rho bit-identical to a fresh device setup of the new model and within 1e-12 of the oracle's (test_equilibration_matches_oracle);
    x, y and the reported solution untouched by the call; after iterate(1) the state of the setup + warm_start route."""
    from pympc_amd import qp_build
    kw = golden_kwargs(load_golden(name))
    new = new_model(kw)
    kwn = with_model(kw, new)
    with _quiet():
        with forced(backend=tag):
            K = controller(kw); K.setup()
            bp = K.prob.batch_problem
            x0, z0, y0 = bp.iterate_state()
            xs0, ys0, i0 = bp.solution()
            K.update_model(solve=False, **new)
            x1, _, y1 = bp.iterate_state()
            xs1, ys1, i1 = bp.solution()
            assert np.array_equal(x0, x1) and np.array_equal(y0, y1)
            assert np.array_equal(xs0, xs1) and np.array_equal(ys0, ys1) and _info(i0[0]) == _info(i1[0])
            # the QP the device now holds
            Kh = controller(kwn); Kh.x0_rh, Kh.uminus1_rh = np.copy(Kh.x0), np.copy(Kh.uminus1)
            Ph, qh, Ah, lh, uh = qp_build.build_qp(Kh)[:5]
            P, q, A, l, u = bp.export_qp()
            U = sp.triu(Ph).toarray()
            assert np.array_equal(P[0], U + np.triu(U, 1).T) and np.array_equal(A[0], Ah.toarray())
            assert np.allclose(q[0], qh, rtol=2e-15, atol=1e-300)
            assert np.array_equal(l[0], np.clip(lh, -1e30, 1e30)) and np.array_equal(u[0], np.clip(uh, -1e30, 1e30))
            # scaling
            Kf = controller(kwn); Kf.setup(solve=False)
            bf = Kf.prob.batch_problem
            for a, b in zip(bp.scaling(), bf.scaling()):
                assert np.array_equal(a, b)
            Ko = controller(kwn, oracle=True); Ko.setup(solve=False)
            D, E, c, rho = bp.scaling()
            Do, Eo, co = Ko.prob.scaling()
            assert rel(D[0], Do) < 1e-12 and rel(E[0], Eo) < 1e-12 and abs(c[0] - co) / co < 1e-12
            assert rho[0] == 0.1
            # one iteration from the kept iterate = one iteration of the setup + warm_start route
            Kf.prob.warm_start(x=x0[0], y=y0[0])
            bp.iterate(1); bf.iterate(1)
            for a, b in zip(bp.iterate_state(), bf.iterate_state()):
                assert np.array_equal(a, b)


@pytest.mark.parametrize('name,tag', CASES, ids=IDS)
def test_solve_after_update_model(name, tag):
    """Default eps: x, y and every mpcqp_info field bit-identical to setup + warm_start + solve on the device; status, iter, rho_updates equal to
    and x within 1e-6 of the oracle's (fresh setup, warm start from the same iterate) -- the assertions of test_default_tolerance_solve_matches_oracle.
    eps 1e-9: u0 within 1e-6 max(|u|, 1e-3) of the oracle's."""
    kw = golden_kwargs(load_golden(name))
    new = new_model(kw)
    kwn = with_model(kw, new)
    with _quiet():
        with forced(backend=tag):
            K = controller(kw); K.setup()
            x0, _, y0 = K.prob.batch_problem.iterate_state()
            K.update_model(**new)
            Kf = controller(kwn); Kf.setup(solve=False)
            Kf.prob.warm_start(x=x0[0], y=y0[0])
            Kf.solve()
            assert np.array_equal(K.res.x, Kf.res.x) and np.array_equal(K.res.y, Kf.res.y)
            assert _res_info(K.res) == _res_info(Kf.res)
            Ko = controller(kwn, oracle=True); Ko.setup(solve=False)
            Ko.prob.warm_start(x=x0[0], y=y0[0])
            Ko.solve()
            assert K.res.info.status == Ko.res.info.status and K.res.info.iter == Ko.res.info.iter
            assert K.res.info.rho_updates == Ko.res.info.rho_updates
            assert rel(K.res.x, Ko.res.x) < 1e-6
            # tight tolerance
            tight = dict(eps_abs=1e-9, eps_rel=1e-9)
            Kt = controller(with_model(kw, tight), max_iter=200000); Kt.setup()
            xt, _, yt = Kt.prob.batch_problem.iterate_state()
            Kt.update_model(**new)
            Kot = controller(with_model(kwn, tight), oracle=True, max_iter=200000); Kot.setup(solve=False)
            Kot.prob.warm_start(x=xt[0], y=yt[0])
            Kot.solve()
            assert Kt.res.info.status == 'solved' and Kot.res.info.status == 'solved'
            uo = Kot.output()
            assert np.abs(Kt.output() - uo).max() <= 1e-6 * max(np.abs(uo).max(), 1e-3)


def _batch_kws(B, seed0=700):
    from pympc_amd import fixtures
    return [fixtures.random_lti(seed0 + i) for i in range(B)]


def _solution_bytes(bp):
    x, y, info = bp.solution()
    return x, y, [_info(i) for i in info]


@pytest.mark.parametrize('tag', ['sweeps', 'bcr', 'bcr8'])
def test_batch_with_a_different_model_per_instance_and_only_some_fields(tag):
    B = 6
    kws = _batch_kws(B)
    news = [new_model(kw, seed=10 + i) for i, kw in enumerate(kws)]
    fields = ('Bd', 'Qx', 'umax', 'Dumin')
    stack = lambda k: np.stack([n[k] for n in news])
    with _quiet():
        with forced(backend=tag):
            K = stacked_batch(kws); K.setup()
            K.update(np.stack([0.9 * np.asarray(kw['x0']) for kw in kws]))        # a warm solve: the iterate is not the cold start's
            x0, _, y0 = K.prob.iterate_state()
            u_before = K.prob.u0()
            K.update_model(solve=False, **{k: stack(k) for k in fields})
            assert np.array_equal(K.prob.u0(), u_before)
            K.solve()
            Kf = stacked_batch([dict(kw, **{k: n[k] for k in fields}, x0=0.9 * np.asarray(kw['x0'])) for kw, n in zip(kws, news)]); Kf.setup(solve=False)
            Kf.prob.warm_start(x0, y0)
            Kf.solve()
            a, b = _solution_bytes(K.prob), _solution_bytes(Kf.prob)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
            assert all(i[0] == 1 for i in a[2])
            for k in fields:
                assert np.array_equal(getattr(K, k), stack(k))


def test_shared_factor_survives_a_model_update():
    """One model in every instance, then one NEW model in every instance: the whole batch shares instance 0's factor again, and the results are
    those of a batch that never shares (MPCQP_TUNE_NO_SHARE)."""
    from pympc_amd import fixtures, _lib
    B = 8
    kw = fixtures.random_lti(41, nx=20, nu=8, Np=12, xbox=3.0)                   # 32 x 32 stages: the streaming backend
    new = new_model(kw, seed=5)
    rng = np.random.default_rng(9)
    xs = np.asarray(kw['x0'])[None] + 0.05 * rng.standard_normal((B, 20))
    out = {}
    with _quiet():
        for tuning in (0, _lib.TUNE_NO_SHARE):
            K = stacked_batch([kw] * B, tuning=tuning); K.setup()
            if not tuning:
                assert K.share_factor() == B
            K.update(xs)
            K.update_model(Ad=new['Ad'], Bd=new['Bd'], QDu=new['QDu'], solve=False)
            if not tuning:
                assert K.share_factor() == B
            K.solve()
            first = _solution_bytes(K.prob)
            K.update(0.9 * xs)
            out[tuning] = (first, _solution_bytes(K.prob))
        for a, b in zip(out[0], out[_lib.TUNE_NO_SHARE]):
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


@pytest.mark.parametrize('polish', [False, True])
@pytest.mark.parametrize('name', ['cart_pole', 'random_12_4_30', 'random_20_8_12_hard'])
def test_step_host_and_polish_after_update_model(name, polish):
    """The paths that follow: MPCController.update() (mpcqp_step_host) after update_model(solve=False), without and with polish=True, equals the
    same call on a freshly set-up handle that was warm-started with the same iterate."""
    kw = golden_kwargs(load_golden(name))
    new = new_model(kw)
    x1 = 0.95 * np.asarray(kw['x0'], dtype=float)
    with _quiet():
        K = controller(kw, polish=polish); K.setup()
        x0, _, y0 = K.prob.batch_problem.iterate_state()
        K.update_model(solve=False, **new)
        K.update(x1)
        Kf = controller(with_model(kw, new), polish=polish); Kf.setup(solve=False)
        Kf.prob.warm_start(x=x0[0], y=y0[0])
        Kf.update(x1)
        assert np.array_equal(K.res.x, Kf.res.x) and np.array_equal(K.res.y, Kf.res.y)
        assert _res_info(K.res) == _res_info(Kf.res) and K.res.info.status_polish == Kf.res.info.status_polish
        assert K.res.info.status == 'solved'
        if polish:
            assert K.res.info.status_polish in (1, -1)


def test_raw_vector_mode_keeps_q_l_u():
    """A problem set up from P, q, A, l, u (mpcqp_setup_csc: raw-vector mode): update_model(Ad, Bd) keeps the vectors, and the next solve is that of a
    fresh problem set up from the new matrices with the same vectors and warm-started."""
    from pympc_amd import qp_build
    from pympc_amd.solver import DeviceProblem
    kw = golden_kwargs(load_golden('random_12_4_30'))
    new = {k: v for k, v in new_model(kw).items() if k in ('Ad', 'Bd')}
    build = lambda kws: (lambda K: qp_build.build_qp(K)[:5])(controller(kws))
    P, q, A, l, u = build(kw)
    Pn, qn, An, ln, un = build(with_model(kw, new))
    assert np.array_equal(q, qn) and np.array_equal(l, ln) and np.array_equal(u, un)      # (only A changes with Ad, Bd)
    st = dict(eps_abs=1e-3, eps_rel=1e-3)
    D = DeviceProblem(); D.setup(P, q, A, l, u, **st)
    r0 = D.solve()
    x0, _, y0 = D.batch_problem.iterate_state()
    D.update_model(**new)
    _, q1, A1, l1, u1 = D.batch_problem.export_qp()
    assert np.array_equal(A1[0], An.toarray()) and np.array_equal(q1[0], q)
    assert np.array_equal(l1[0], np.clip(l, -1e30, 1e30)) and np.array_equal(u1[0], np.clip(u, -1e30, 1e30))
    r1 = D.solve()
    F = DeviceProblem(); F.setup(Pn, q, An, l, u, **st)
    F.warm_start(x=x0[0], y=y0[0])
    rf = F.solve()
    assert np.array_equal(r1.x, rf.x) and np.array_equal(r1.y, rf.y) and _res_info(r1) == _res_info(rf)
    assert r0.info.status == 'solved' and r1.info.status == 'solved'


# ---- mpcqp_mpc_loop_tv ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [8, 1100])
@pytest.mark.parametrize('hold', [1, 3])
def test_loop_tv_is_the_segment_sequence_written_on_the_host(B, hold):
    """run(model_traj=) = per entry update_model(entry, solve=False) and run(min(hold, rest)) on the advanced trajectories, bit for bit -- at a
    batch that is resident at once and at one that goes through the persistent queue; nsteps is not a multiple of hold."""
    nsteps = 7
    nm = (nsteps + hold - 1) // hold
    kws = _batch_kws(B, seed0=3000)
    sched = [model_schedule(kw['Ad'], kw['Bd'], nm, seed=i) for i, kw in enumerate(kws)]
    Adt, Bdt = np.stack([s[0] for s in sched], axis=1), np.stack([s[1] for s in sched], axis=1)      # [nm, B, ...]
    wn = 0.01 * np.random.default_rng(4).standard_normal((nsteps, B, 12))
    with _quiet():
        Kd = stacked_batch(kws); Kd.setup()
        Ks = stacked_batch(kws); Ks.setup()
        tr = Kd.run(nsteps, w=wn, model_traj=(Adt, Bdt, hold))
        xs, us, ss, its = [], [], [], []
        for s in range(nm):
            k0, k1 = s * hold, min(nsteps, (s + 1) * hold)
            Ks.update_model(Ad=Adt[s], Bd=Bdt[s], solve=False)
            t = Ks.run(k1 - k0, w=wn[k0:k1])
            xs.append(t['x'][:-1] if s < nm - 1 else t['x']); us.append(t['u']); ss.append(t['status']); its.append(t['iter'])
        assert np.array_equal(tr['x'], np.concatenate(xs)) and np.array_equal(tr['u'], np.concatenate(us))
        assert np.array_equal(tr['status'], np.concatenate(ss)) and np.array_equal(tr['iter'], np.concatenate(its))
        a, b = _solution_bytes(Kd.prob), _solution_bytes(Ks.prob)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
        assert np.array_equal(Kd.Ad, Adt[nm - 1]) and np.array_equal(Kd.Bd, Bdt[nm - 1])
        # the plant followed the model in force
        for k in range(nsteps):
            e = k // hold
            xn = np.einsum('bij,bj->bi', Adt[e], tr['x'][k]) + np.einsum('bij,bj->bi', Bdt[e], tr['u'][k]) + wn[k]
            assert np.allclose(xn, tr['x'][k + 1], rtol=1e-13, atol=1e-14)
        if B > 1000:
            assert Kd.prob.carry_stats()[2] >= 1                                 # the persistent queue was in use


@pytest.mark.parametrize('hold', [1, 3])
@pytest.mark.parametrize('name', ['point_mass', 'cart_pole', 'quadcopter_nc', 'random_12_4_30'])
def test_loop_tv_matches_the_oracle_stepped_in_python(name, hold):
    """eps 1e-9, the tolerances of test_closed_loop_matches_oracle: every applied input within 1e-6 max(|u|, 1e-3) of the oracle's, every step of both
    'solved'.  The schedule is tests/ltv_models.model_schedule at amplitude 0.03: a seeded smooth perturbation of Ad, Bd under which the oracle ALONE
    (its own plant, CPU only) ends all 14 steps 'solved' on these fixtures at hold 1 and 3 -- checked at 0.03 and 0.1 when the test was written.  The
    oracle is stepped with the device's states and inputs, like the stepwise controller of test_device_loop_matches_stepwise_api."""
    nsteps = 14
    nm = (nsteps + hold - 1) // hold
    kw = golden_kwargs(load_golden(name))
    kt = with_model(kw, dict(eps_abs=1e-9, eps_rel=1e-9))
    Adt, Bdt = model_schedule(kw['Ad'], kw['Bd'], nm, amp=0.03)
    with _quiet():
        Kd = stacked_batch([kt], eps_abs=1e-9, eps_rel=1e-9, max_iter=100000); Kd.setup()
        Ko = controller(kt, oracle=True, max_iter=100000); Ko.setup()
        assert Ko.res.info.status == 'solved'
        tr = Kd.run(nsteps, model_traj=(Adt[:, None], Bdt[:, None], hold))
        for k in range(nsteps):
            if k % hold == 0:
                Ko.update_model(Ad=Adt[k // hold], Bd=Bdt[k // hold], solve=False)
            uo = Ko.output()
            assert np.abs(tr['u'][k, 0] - uo).max() <= 1e-6 * max(np.abs(uo).max(), 1e-3), k
            xn = Adt[k // hold] @ tr['x'][k, 0] + Bdt[k // hold] @ tr['u'][k, 0]
            assert np.allclose(xn, tr['x'][k + 1, 0], rtol=1e-13, atol=1e-14)
            Ko.update(tr['x'][k + 1, 0], tr['u'][k, 0])
            assert Ko.res.info.status == 'solved' and tr['status'][k, 0] == 1, k
        assert np.abs(Kd.output()[0] - Ko.output()).max() <= 1e-6 * max(np.abs(Ko.output()).max(), 1e-3)


def test_loop_tv_with_device_resident_buffers_and_no_schedule():
    """Everything in device memory (torch tensors): the same numbers as with host arrays; model_traj=None is mpcqp_mpc_loop."""
    import torch
    B, nsteps, hold = 5, 6, 2
    kws = _batch_kws(B, seed0=3500)
    sched = [model_schedule(kw['Ad'], kw['Bd'], 3, seed=i) for i, kw in enumerate(kws)]
    Adt, Bdt = np.stack([s[0] for s in sched], axis=1), np.stack([s[1] for s in sched], axis=1)
    with _quiet():
        Kh = stacked_batch(kws); Kh.setup()
        Kd = stacked_batch(kws); Kd.setup()
        th = Kh.run(nsteps, model_traj=(Adt, None, hold))
        dev = lambda a, dt=torch.float64: torch.zeros(a.shape, dtype=dt, device='cuda')
        out = [dev(th['x']), dev(th['u']), dev(th['status'], torch.int32), dev(th['iter'], torch.int32)]
        Kd.prob.mpc_run(nsteps, out=out, model_traj=(torch.as_tensor(Adt, device='cuda'), None, hold))
        Kd.prob.synchronize()
        for a, k in zip(out, ('x', 'u', 'status', 'iter')):
            assert np.array_equal(a.cpu().numpy(), th[k]), k
        # no schedule: the plain loop
        a, b = Kh.run(3), Kd.prob.mpc_run(3, model_traj=None)
        assert np.array_equal(a['x'], b[0]) and np.array_equal(a['u'], b[1])


# ---- errors ----------------------------------------------------------------------------------------------------------------------
def test_error_codes():
    from pympc_amd import _lib
    from pympc_amd.solver import BatchProblem
    L = _lib.load()
    assert _lib.has_model_update(L)
    kws = _batch_kws(2)
    bp = BatchProblem(2, 12, 4, 30)
    Ad = np.ascontiguousarray(np.stack([kw['Ad'] for kw in kws]))
    M = _lib.Model()
    M.Ad = Ad.ctypes.data_as(C.POINTER(C.c_double))
    assert L.mpcqp_update_model(bp._h, C.byref(M)) == ERR_STATE                   # before setup
    assert L.mpcqp_update_model(bp._h, None) == ERR_ARG
    assert L.mpcqp_update_model(bp._h, C.byref(_lib.Model())) == ERR_ARG          # no field given
    assert L.mpcqp_update_model(None, C.byref(M)) == ERR_ARG
    with pytest.raises(TypeError):
        bp.update_model(Cd=Ad)
    with pytest.raises(ValueError):
        bp.update_model()
    with _quiet():
        K = stacked_batch(kws); K.setup()
    h = K.prob._h
    assert L.mpcqp_update_model(h, None) == ERR_ARG and L.mpcqp_update_model(h, C.byref(_lib.Model())) == ERR_ARG
    before = _solution_bytes(K.prob)
    nsteps, B = 5, 2
    Adt = np.ascontiguousarray(np.broadcast_to(Ad, (3, B, 12, 12)))
    outs = [np.empty((nsteps + 1, B, 12)), np.empty((nsteps, B, 4)), np.empty((nsteps, B), dtype=np.int32), np.empty((nsteps, B), dtype=np.int32)]
    io = _lib.Loop()
    io.x_traj, io.u_traj, io.status_traj, io.iter_traj = (o.ctypes.data for o in outs)

    def traj(**kw):
        mt = _lib.ModelTraj()
        mt.struct_size, mt.hold, mt.nmodels, mt.Ad = C.sizeof(_lib.ModelTraj), 2, 3, Adt.ctypes.data
        for k, v in kw.items():
            setattr(mt, k, v)
        return mt
    call = lambda io, mt: L.mpcqp_mpc_loop_tv(h, nsteps, C.byref(io), C.byref(mt))
    assert call(io, traj(struct_size=C.sizeof(_lib.ModelTraj) - 8)) == ERR_ARG
    assert call(io, traj(hold=0)) == ERR_ARG
    assert call(io, traj(nmodels=2)) == ERR_ARG                                   # ceil(5 / 2) = 3 entries needed
    assert call(io, traj(Ad=None)) == ERR_ARG                                     # neither Ad nor Bd
    x_true, Cm, Lg = np.zeros((B, 12)), np.zeros((B, 1, 12)), np.zeros((B, 12, 1))
    io_fb = _lib.Loop()
    io_fb.x_traj, io_fb.u_traj, io_fb.status_traj, io_fb.iter_traj = (o.ctypes.data for o in outs)
    io_fb.ny, io_fb.C, io_fb.Lgain, io_fb.x_true = 1, Cm.ctypes.data, Lg.ctypes.data, x_true.ctypes.data
    assert call(io_fb, traj()) == ERR_UNSUPPORTED
    assert b'output feedback' in L.mpcqp_last_error()
    after = _solution_bytes(K.prob)
    assert np.array_equal(before[0], after[0]) and before[2] == after[2]         # a refused call changes nothing
    assert call(io, traj()) == 0 and (outs[2] == 1).all()                        # ... and the handle is still good
    with pytest.raises(NotImplementedError):
        K.prob.mpc_run(2, model_traj=(Adt, None, 1), estimator=dict(C=Cm, L=Lg, x_true=x_true))
    with pytest.raises(RuntimeError):
        K.prob.mpc_run(5, model_traj=(Adt[:2], None, 2))


@pytest.mark.parametrize('tag', ['sweeps', 'dense', 'bcr', 'bcr8'])
def test_indefinite_qx_reports_non_convex(tag):
    """Qx = QxN = -1e6 I makes the reduced KKT matrix of the cart pole indefinite (21 negative eigenvalues with the scaling of |Qx|): the
    factorization of update_model meets a non-positive pivot and reports it as setup's does -- status 'problem non convex', iter 0, at once.  The
    iterate is kept, so a good model given before the next solve clears the verdict and solves."""
    kw = golden_kwargs(load_golden('cart_pole'))
    with _quiet():
        with forced(backend=tag):
            K = controller(kw); K.setup()
            bp = K.prob.batch_problem
            K.update_model(Qx=-1e6 * np.eye(4), QxN=-1e6 * np.eye(4), solve=False)
            i = bp.infos()[0]
            assert (i.status, i.iter) == (NON_CVX, 0)
            assert bp.status_string(i.status) == 'problem non convex'
            K.update_model(Qx=kw['Qx'], QxN=kw['QxN'], solve=False)
            assert bp.infos()[0].status != NON_CVX
            K.solve()
            assert K.res.info.status == 'solved'
