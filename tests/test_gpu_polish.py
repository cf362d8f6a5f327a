"""Solution polishing on the device (include/mpcqp_polish.h, pympc_amd/csrc/mpcqp_polish.h) against the certified optima of the golden
fixtures and against the numpy restatement of OSQP's polish (tests/polish_ref.py), on every KKT backend, in mixed batches, through the
drop-in class and the reference seam."""
import warnings

import numpy as np
import pytest

from util import golden_names, load_golden, golden_kwargs, apply_attrs, rel1, golden_backends, repeated, stacked_batch, point_mass_batch
from polish_ref import golden_qp, check_against_spec, ACCEPTED, EXACT_SCALED as EXACT

pytestmark = pytest.mark.gpu

EPS = 1e-3


def _opt(name):
    import os
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'opt_%s.npz' % name))


def _ctrl(kw, eps=EPS, **settings):
    from pympc_amd import MPCController
    from util import KW
    attrs = getattr(kw, 'attrs', {})
    kw = KW(kw); kw.attrs = attrs
    kw.update(eps_abs=eps, eps_rel=eps)
    K = apply_attrs(MPCController(**kw), kw)
    K.solver_settings = dict(max_iter=200000, **settings)
    return K


def _golden_ctrl(name, **settings):
    return _ctrl(golden_kwargs(load_golden(name)), **settings)


# ---- 1. accuracy at the reference tolerance ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', golden_names())
def test_polish_at_pympcs_tolerance(name):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        K0 = _golden_ctrl(name); K0.setup()
        K = _golden_ctrl(name, polish=True); K.setup()
    opt = _opt(name)
    assert K.res.info.status == 'solved'
    sp = K.res.info.status_polish
    if sp == 1:
        assert K.res.info.pri_res < K0.res.info.pri_res or K.res.info.dua_res < K0.res.info.dua_res
    else:
        assert sp == -1
        assert np.array_equal(K.res.x, K0.res.x) and np.array_equal(K.res.y, K0.res.y)
        assert K.res.info.obj_val == K0.res.info.obj_val
    if name in ACCEPTED:
        assert sp == 1, name                        # accepted from the oracle's iterate on the CPU: the device must accept too
    if name in EXACT:
        assert rel1(K.res.x, opt['x']) <= 1e-8, (name, rel1(K.res.x, opt['x']))
        u0 = K.output()
        assert np.abs(u0 - opt['u0']).max() <= 1e-8 * max(1.0, np.abs(opt['u0']).max()), name
        assert rel1(K0.res.x, opt['x']) > 1e-8       # what polishing changed


def test_named_fixtures_include_the_headline_shape_and_the_cart_pole():
    assert 'random_12_4_30' in EXACT and 'cart_pole' in ACCEPTED


# ---- 2. device against the numpy spec ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', golden_names())
def test_device_polish_is_the_spec(name):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        K = _golden_ctrl(name); K.setup()
    bp = K.prob.batch_problem
    if K.res.info.status != 'solved':
        pytest.fail('not solved')
    check_against_spec(bp)


# ---- 3. every backend, grouped stages, wide stages ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['random_12_4_30', 'point_mass', 'small_mimo', 'quadcopter_nodu', 'random_5_3_8_nc'])
def test_polish_agrees_across_backends_and_leaves_the_handle_factor(name):
    from pympc_amd.solver import forced_settings
    res = {}
    for be in golden_backends(name):
        with forced_settings(backend=be):
            K = _golden_ctrl(name); K.setup()
        bp = K.prob.batch_problem
        rhs = np.random.default_rng(0).standard_normal((1, bp.n))
        before = bp.kkt_solve(rhs)
        st = check_against_spec(bp)
        after = bp.kkt_solve(rhs)
        assert np.array_equal(before, after), be          # the handle's own factor is untouched
        res[be] = (st[0], bp.solution()[0][0])
    base = res['sweeps']
    for be, (st, x) in res.items():
        assert st == base[0], be
        if st == 1:
            assert rel1(x, base[1]) <= 1e-10, (be, rel1(x, base[1]))


def _kw(**over):
    from pympc_amd import fixtures
    from util import KW
    kw = KW(fixtures.cart_pole(Np=over.pop('Np', 20)))
    kw.update(over)
    return kw


@pytest.mark.parametrize('make', [
    lambda: golden_kwargs(load_golden('cart_pole_kalman')),                              # grouped small stages (4, 1, 200)
    lambda: _kw(Np=150, Nc=75),                                                           # grouped, held input (4, 1, 150, 75)
    lambda: __import__('pympc_amd').fixtures.random_lti(3, nx=30, nu=10, Np=8),          # stages 33..64 wide
    lambda: __import__('pympc_amd').fixtures.random_lti(4, nx=60, nu=20, Np=4),          # stages 65..128 wide
    lambda: _kw(Np=20, Nc=5),                                                             # held input, bordered factor
], ids=['grouped', 'grouped_held', 'wide64', 'wide128', 'held'])


def test_polish_on_grouped_and_wide_layouts(make):
    from util import KW
    kw = make()
    kw = kw if isinstance(kw, KW) else KW(kw)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        K = _ctrl(kw); K.setup()
    assert K.res.info.status == 'solved'
    bp = K.prob.batch_problem
    rhs = np.random.default_rng(1).standard_normal((1, bp.n))
    before = bp.kkt_solve(rhs)
    check_against_spec(bp)
    assert np.array_equal(before, bp.kkt_solve(rhs))


def test_shared_factor_map_survives_polishing():
    from pympc_amd import BatchMPCController, fixtures
    kw = fixtures.random_lti(7)
    B = 8
    st = lambda a: np.stack([np.asarray(a, dtype=float)] * B)
    K = BatchMPCController(**repeated(kw, B, eps_feas=1e6, eps_abs=EPS, eps_rel=EPS, backend='sweeps', polish=True))
    K.setup(solve=False)
    n = K.share_factor()
    assert n == B
    rhs = np.random.default_rng(2).standard_normal((B, K.prob.n))
    before = K.prob.kkt_solve(rhs)
    K.update(st(kw['x0']) * np.linspace(0.5, 1.0, B)[:, None])
    assert np.all(K.prob.polish_status() != 0)
    assert np.array_equal(before, K.prob.kkt_solve(rhs))


# ---- 4. mixed batch ---------------------------------------------------------------------------------------------------------------------
def _point_mass_batch(polish):
    K, _ = point_mass_batch(eps_abs=EPS, eps_rel=EPS, polish=polish)      # (instance 2 infeasible: tests/test_gpu_parity.py's recipe)
    K.setup()
    return K


def test_mixed_batch_polishes_the_solved_and_leaves_the_infeasible():
    K0, K = _point_mass_batch(False), _point_mass_batch(True)
    st = K.prob.polish_status()
    assert K.status()[2] == 'primal infeasible'
    assert st[2] == 0 and all(st[b] != 0 for b in (0, 1, 3, 4)), st
    x0, y0, i0 = K0.prob.solution()
    x1, y1, i1 = K.prob.solution()
    assert np.array_equal(x0[2], x1[2], equal_nan=True) and np.array_equal(y0[2], y1[2], equal_nan=True)
    assert bytes(i0[2]) == bytes(i1[2])
    assert np.array_equal(K.output()[2], K0.output()[2])
    assert all(K0.prob.polish_status() == 0)


# ---- 5. warm start ----------------------------------------------------------------------------------------------------------------------
def test_accepted_polish_becomes_the_warm_start():
    K = _golden_ctrl('random_12_4_30', polish=True)
    K.setup()
    bp = K.prob.batch_problem
    assert bp.polish_status()[0] == 1
    x, y, info = bp.solution()
    xi, zi, yi = bp.iterate_state()
    assert np.array_equal(xi, x) and np.array_equal(yi, y)
    P, q, A, l, u = bp.export_qp()
    assert np.allclose(zi[0], np.clip(A[0] @ x[0], l[0], u[0]), rtol=0, atol=1e-12 * max(1.0, np.abs(x).max()))
    # the next solve (same data) starts at the polished point: it terminates at its first check, still at the optimum
    bp.solve_async()
    x2, _, info2 = bp.solution()
    assert info2[0].status == 1 and info2[0].iter == bp.settings.check_termination
    assert rel1(x2[0], _opt('random_12_4_30')['x']) <= 1e-8


# ---- 6. rejection -----------------------------------------------------------------------------------------------------------------------
def test_rejected_polish_changes_nothing():
    K0 = _golden_ctrl('random_12_4_30'); K0.setup()
    K = _golden_ctrl('random_12_4_30', polish=True, delta=10.0, polish_refine_iter=0); K.setup()
    bp, bp0 = K.prob.batch_problem, K0.prob.batch_problem
    assert bp.polish_status()[0] == -1
    for a, b in zip(bp.solution(), bp0.solution()):
        assert bytes(a) == bytes(b) if not isinstance(a, np.ndarray) else np.array_equal(a, b)
    for a, b in zip(bp.iterate_state(), bp0.iterate_state()):
        assert np.array_equal(a, b)
    assert K.res.info.status_polish == -1


# ---- 7. drop-in ------------------------------------------------------------------------------------------------------------------------
def test_drop_in_controller_and_seam_return_the_optimum():
    from pympc_amd.solver import DeviceProblem
    opt = _opt('random_12_4_30')
    K = _golden_ctrl('random_12_4_30', polish=True); K.setup()
    assert K.res.info.status_polish == 1
    assert np.abs(K.output() - opt['u0']).max() <= 1e-8 * max(1.0, np.abs(opt['u0']).max())
    P, q, A, l, u = golden_qp(load_golden('random_12_4_30'))
    prob = DeviceProblem()
    prob.setup(P, q, A, l, u, eps_abs=EPS, eps_rel=EPS, polish=True)
    res = prob.solve()
    assert res.info.status == 'solved' and res.info.status_polish == 1
    assert rel1(res.x, opt['x']) <= 1e-8
    prob.update_settings(polish=False)
    assert prob.solve().info.status_polish == 0
    prob.update_settings(polish=True)
    assert prob.solve().info.status_polish == 1


def test_device_loop_refuses_polishing():
    from pympc_amd import BatchMPCController, fixtures
    kw = fixtures.point_mass()
    K = BatchMPCController(**repeated(kw, 2, uminus1=None, eps_feas=kw.get('eps_feas', 1e6), polish=True))      # (u_{-1}: the constructor's default)
    K.setup()
    with pytest.raises(NotImplementedError):
        K.run(3)
    K.prob.update_settings(polish=False)
    K.run(3)
    assert np.all(K.prob.polish_status() == 0)


def test_polish_off_is_bit_identical_to_never_mentioning_it():
    from pympc_amd import fixtures
    kw = fixtures.cart_pole()
    outs = []
    for settings in (dict(), dict(polish=False, delta=1e-6, polish_refine_iter=3)):
        K = _ctrl(kw, **settings)
        K.setup()
        x, us = np.array(kw['x0'], dtype=float), []
        for _ in range(6):
            u = K.output()
            us.append(u.copy())
            x = kw['Ad'] @ x + kw['Bd'] @ u
            K.update(x, u)
            assert K.res.info.status_polish == 0
        outs.append((np.array(us), K.res.x.copy(), K.res.y.copy()))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


def test_polish_inside_mpc_step_and_the_stepwise_controller():
    from pympc_amd import fixtures
    kw = _kw()
    K = _ctrl(kw, polish=True)
    K.setup()
    x = np.array(kw['x0'], dtype=float)
    for _ in range(4):
        u = K.output()
        x = kw['Ad'] @ x + kw['Bd'] @ u
        K.update(x, u)
        assert K.res.info.status == 'solved' and K.res.info.status_polish in (1, -1)


# ---- 8. the headline shape ---------------------------------------------------------------------------------------------------------------
def _random_batch(idx, eps, **settings):
    from pympc_amd import fixtures
    K = stacked_batch([fixtures.random_lti(int(i)) for i in idx], eps_feas=1e6, eps_abs=eps, eps_rel=eps, max_iter=400000, **settings)
    K.setup()
    return K


def test_headline_batch_1024_x_12_4_30():
    B = 1024
    K = _random_batch(range(B), EPS, polish=True)
    st = K.prob.polish_status()
    assert all(s == 'solved' for s in K.status())
    assert np.all(st != 0) and np.mean(st == 1) > 0.9, np.mean(st == 1)
    sample = np.arange(0, B, B // 64)
    # the same 64 instances unpolished, polished on demand against the spec
    K64 = _random_batch(sample, EPS)
    st64 = check_against_spec(K64.prob)
    assert np.array_equal(st64, st[sample])
    # polished u0 against the optimum (the same instances solved to eps 1e-11)
    Kopt = _random_batch(sample, 1e-11)
    u_opt = Kopt.prob.u0()
    u_pol = K.prob.u0()[sample]
    for j in np.flatnonzero(st[sample] == 1):
        assert np.abs(u_pol[j] - u_opt[j]).max() <= 1e-8 * max(1.0, np.abs(u_opt[j]).max()), j
