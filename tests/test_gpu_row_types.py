"""Every KKT backend on batches whose instances mix constraint-row types (tests/row_patterns.py): loose, equality and inequality rows
of the state box, the input box and the Delta-u bounds, different from instance to instance, and row types changed after setup
through the raw seam.  Per instance against the reduced KKT matrix built from the row-type rule and against the oracle; the instance
-> workgroup map and the closed loop's carry must not change a result.
Run on the GPU box with:  python -m pytest tests/test_gpu_row_types.py -m gpu
"""
import functools
import warnings

import numpy as np
import pytest

import row_patterns as rp
from polish_ref import check_against_spec
from util import eligible_backends, rel, info_tuple, carry_on_and_off

pytestmark = pytest.mark.gpu

# (nx, nu, Np, Nc, soft) -> the path it targets
SHAPES = {
    '12_4_30': (12, 4, 30, None, True),            # compile-time dimensions, schedule 31
    '10_3_30': (10, 3, 30, None, True),            # generic, schedule 31
    '6_2_20': (6, 2, 20, None, True),              # schedule 21
    '12_4_10': (12, 4, 10, None, True),            # schedule 11
    '3_1_30': (3, 1, 30, None, True),              # dense-eligible
    '4_1_20': (4, 1, 20, None, True),
    '20_8_12': (20, 8, 12, None, True),            # cfg-5's compile-time 32-wide instantiation
    '18_6_12': (18, 6, 12, None, True),            # generic 32-wide
    '30_10_8': (30, 10, 8, None, True),            # wide
    '60_20_4': (60, 20, 4, None, True),            # huge
    '3_1_200': (3, 1, 200, None, True),            # grouped
    '4_1_150_nc75': (4, 1, 150, 75, True),
    '12_4_30_nc10': (12, 4, 30, 10, True),         # bordered
    '12_4_30_hard': (12, 4, 30, None, False),      # hard state box
}


CASES = [(s, t) for s in SHAPES for t in eligible_backends(*SHAPES[s][:4])]
CASE_IDS = ['%s-%s' % c for c in CASES]
FLIPPED = (3, 6)
_cache = {}
_oracle = functools.partial(rp.oracle, quiet=True)


def _kws(sid):
    if sid not in _cache:
        nx, nu, Np, Nc, soft = SHAPES[sid]
        _cache[sid] = rp.batch(nx, nu, Np, Nc, soft)
    return _cache[sid]


def _dims(sid):
    nx, nu, Np, Nc, _ = SHAPES[sid]
    return (Np + 1) * nx, (Nc or Np) * nu


def _dev(kws, tag, eps, solve=True, **kw):
    from pympc_amd import BatchMPCController
    from pympc_amd.solver import forced_settings
    with forced_settings(backend=tag), warnings.catch_warnings():
        warnings.simplefilter('ignore')
        K = BatchMPCController(**rp.stack(kws, eps_abs=eps, eps_rel=eps, max_iter=400000, **kw))
        K.setup(solve=solve)
    return K


def _oracle_solves(sid, eps):
    key = (sid, 'solve', eps)
    if key not in _cache:
        _cache[key] = [(k.res.info.status, k.res.info.iter, k.res.info.rho_updates, k.res.x.copy()) for k in (_oracle(kw, eps) for kw in _kws(sid))]
    return _cache[key]


def _oracle_iterates(sid, iters):
    key = (sid, 'iterate', iters)
    if key not in _cache:
        out = []
        for kw in _kws(sid):
            K = _oracle(kw, 1e-3, solve=False)
            K.prob.iterate(iters)
            out.append(K.prob.iterate_state()[:3])
        _cache[key] = out
    return _cache[key]


def _check_kkt(bp, seed=5):
    """kkt_solve with a different right-hand side per instance, each row against its own reduced KKT matrix: backward error
    <= 1e-12 (tests/test_gpu_gaps.py) and forward error <= 1e-8 (tests/test_gpu_backends.py)."""
    rhs = np.random.default_rng(seed).standard_normal((bp.batch, bp.n))
    sol = bp.kkt_solve(rhs)
    assert np.isfinite(sol).all()
    for b in range(bp.batch):
        Km = rp.reduced_kkt(bp, b)
        back = np.abs(Km @ sol[b] - rhs[b]).max() / (np.abs(Km) @ np.abs(sol[b]) + np.abs(rhs[b])).max()
        assert back <= 1e-12, (b, back)
        assert rel(sol[b], np.linalg.solve(Km, rhs[b])) < 1e-8, b


def _check_solves(K, sid, eps, idx=None):
    """eps 1e-3: status, iterations and rho updates as the oracle; eps 1e-10: status and u_seq within 1e-6."""
    n_x, n_u = _dims(sid)
    x, _, info = K.prob.solution()
    ref = _oracle_solves(sid, eps)
    for b in (range(K.B) if idx is None else idx):
        st, it, ru, xo = ref[b]
        assert K.prob.status_string(info[b].status) == st, (b, K.prob.status_string(info[b].status), st)
        if eps >= 1e-3:
            assert (info[b].iter, info[b].rho_updates) == (it, ru), (b, info[b].iter, it, info[b].rho_updates, ru, info[b].rho)
        else:
            uo = xo[n_x:n_x + n_u]
            assert np.abs(x[b][n_x:n_x + n_u] - uo).max() <= 1e-6 * max(1e-3, np.abs(uo).max()), b


def _mode(tag, nx, nu, Np):
    sched = 11 if Np + 1 <= 11 else 21 if Np + 1 <= 21 else 31
    return {'dense': 2, 'bcr': 100 + sched, 'bcr8': 200 + sched, 'bcrt': 200 + sched}.get(tag)


# ---- a. the KKT solve of every instance ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sid,tag', CASES, ids=CASE_IDS)
def test_kkt_solve_on_every_instance(sid, tag):
    nx, nu, Np, Nc, _ = SHAPES[sid]
    kws = _kws(sid)
    assert len({rp.row_types(kw).tobytes() for kw in kws}) > 1          # (the batch mixes row-type patterns)
    K = _dev(kws, tag, 1e-3, solve=False)
    bp = K.prob
    kn = bp.kernel_name(loop=False)
    if _mode(tag, nx, nu, Np) is not None:
        assert int(kn.split(',')[4]) == _mode(tag, nx, nu, Np) and kn.startswith('w8::') == (tag == 'bcr8'), kn
    else:
        assert int(kn.split(',')[4]) < 100 and int(kn.split(',')[4]) != 2, kn
    _check_kkt(bp)
    bp.refactor(); bp.synchronize()
    _check_kkt(bp)


# ---- b. ADMM iterates --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sid,tag', CASES, ids=CASE_IDS)
def test_admm_iterates_match_oracle_per_instance(sid, tag):
    kws = _kws(sid)
    for iters in (1, 7, 40):
        K = _dev(kws, tag, 1e-3, solve=False)
        K.prob.iterate(iters)
        x, z, y = K.prob.iterate_state()
        for b, (xo, zo, yo) in enumerate(_oracle_iterates(sid, iters)):
            assert rel(x[b], xo) < 1e-8 and rel(z[b], zo) < 1e-8, (iters, b, rel(x[b], xo), rel(z[b], zo))
            assert np.abs(y[b] - yo).max() < 1e-8 * max(1.0, np.abs(yo).max()), (iters, b)


# ---- c. solves ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sid,tag', CASES, ids=CASE_IDS)
def test_solves_match_oracle_per_instance(sid, tag):
    kws = _kws(sid)
    for eps in (1e-3, 1e-10):
        K = _dev(kws, tag, eps)
        _check_solves(K, sid, eps)
        assert sum(i.status == 1 for i in K.prob.infos()) >= 7


# ---- d. position independence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sid,tag', CASES, ids=CASE_IDS)
def test_reversed_instance_order_gives_bit_identical_results(sid, tag):
    """the instance -> workgroup map never changes a result."""
    kws = _kws(sid)
    out = []
    for order in (kws, kws[::-1]):
        K = _dev(order, tag, 1e-3)
        x, y, _ = K.prob.solution()
        out.append((x, y, info_tuple(K.prob.infos())) + tuple(K.prob.iterate_state()))
    for a, b in zip(*out):
        assert np.array_equal(a, b[::-1])


# ---- e. row types changed through the seam -----------------------------------------------------------------------------------------------
def _flip_oracles(sid, eps):
    """The flipped instances' oracles through three successive flip_types updates: [(l, u, result) per update] per instance."""
    key = (sid, 'flip', eps)
    if key not in _cache:
        out = {}
        for b in FLIPPED:
            kw, rng = _kws(sid)[b], np.random.default_rng(40 + b)
            Ko, steps = _oracle(kw, eps), []
            for _ in range(3):
                kw, l, u = rp.flip_types(kw, rng)
                Ko.prob.update(l=l, u=u)
                r = Ko.prob.solve()
                steps.append((l, u, (r.info.status, r.info.iter, r.info.rho_updates, r.x.copy())))
            out[b] = steps
        _cache[key] = out
    return _cache[key]


@pytest.mark.parametrize('sid,tag', [c for c in CASES if SHAPES[c[0]][4]], ids=[i for c, i in zip(CASES, CASE_IDS) if SHAPES[c[0]][4]])
def test_row_type_changes_through_the_seam(sid, tag):
    """Three successive flip_types updates of instances 3 and 6 through BatchProblem.update_vectors (the same on the oracle): after
    each, the in-kernel refactorization solves with the new types' reduced KKT matrix, the flipped instances' solves match the oracle
    at both tolerances, and the other instances are bit-identical to a run that gets its unchanged vectors again."""
    kws = _kws(sid)
    n_x, n_u = _dims(sid)
    L0 = np.stack([rp.bounds(kw)[0] for kw in kws])
    U0 = np.stack([rp.bounds(kw)[1] for kw in kws])
    others = [b for b in range(len(kws)) if b not in FLIPPED]
    for eps in (1e-3, 1e-10):
        ref = _flip_oracles(sid, eps)
        Kf, Kn = _dev(kws, tag, eps), _dev(kws, tag, eps)
        L, U = L0.copy(), U0.copy()
        for k in range(3):
            for b in FLIPPED:
                L[b], U[b] = ref[b][k][0], ref[b][k][1]
            for K, (l, u) in ((Kf, (L, U)), (Kn, (L0, U0))):
                K.prob.update_vectors(None, l, u)
                K.prob.solve_async()
            x, y, info = Kf.prob.solution()
            xn, yn, infon = Kn.prob.solution()
            _, _, Ae, le, ue = Kf.prob.export_qp()
            for b in FLIPPED:
                assert np.array_equal(le[b], L[b]) and np.array_equal(ue[b], U[b])
                st, it, ru, xo = ref[b][k][2]
                assert Kf.prob.status_string(info[b].status) == st, (k, b)
                if eps >= 1e-3:
                    assert (info[b].iter, info[b].rho_updates) == (it, ru), (k, b, info[b].iter, it, info[b].rho_updates, ru, info[b].rho)
                else:
                    uo = xo[n_x:n_x + n_u]
                    assert np.abs(x[b][n_x:n_x + n_u] - uo).max() <= 1e-6 * max(1e-3, np.abs(uo).max()), (k, b)
            assert np.array_equal(x[others], xn[others]) and np.array_equal(y[others], yn[others])
            assert np.array_equal(info_tuple(info)[others], info_tuple(infon)[others])
            _check_kkt(Kf.prob, seed=k)


def test_row_type_changes_through_device_problem():
    """The same three updates through DeviceProblem (batch 1, set up from the reference-built P, q, A, l, u) on (12,4,30)."""
    from pympc_amd.solver import DeviceProblem
    kw = _kws('12_4_30')[FLIPPED[0]]
    n_x, n_u = _dims('12_4_30')
    for eps in (1e-3, 1e-10):
        Ko = _oracle(kw, eps)
        dp = DeviceProblem()
        dp.setup(Ko.P, Ko.q, Ko.A, Ko.l, Ko.u, eps_abs=eps, eps_rel=eps, max_iter=400000, warm_start=True)
        r = dp.solve()
        assert (r.info.status, r.info.iter) == (Ko.res.info.status, Ko.res.info.iter)
        for k, (l, u, (st, it, ru, xo)) in enumerate(_flip_oracles('12_4_30', eps)[FLIPPED[0]]):
            dp.update(l=l, u=u)
            r = dp.solve()
            assert r.info.status == st, (k, r.info.status, st)
            if eps >= 1e-3:
                assert (r.info.iter, r.info.rho_updates) == (it, ru), (k, r.info.iter, it)
            else:
                uo = xo[n_x:n_x + n_u]
                assert np.abs(r.x[n_x:n_x + n_u] - uo).max() <= 1e-6 * max(1e-3, np.abs(uo).max()), k
            _check_kkt(dp.batch_problem, seed=k)


# ---- f. the headline kernel in closed loop -----------------------------------------------------------------------------------------------
def test_headline_kernel_closed_loop_on_mixed_patterns():
    """64 mixed (12,4,30) instances on the auto-selected kernel, 10 closed-loop steps at eps 1e-3 with disturbances; the oracle steps
    alongside on 16 of them (test_gpu_gaps.py: test_auto_selected_latency_backend_at_per_gpu_batches_matches_oracle)."""
    from pympc_amd import BatchMPCController
    B = 64
    kws = [rp.draw(s, 12, 4, 30) for s in range(B)]
    assert rp.kinds_present(kws) >= rp.ALL_KINDS
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        K = BatchMPCController(**rp.stack(kws, eps_abs=1e-3, eps_rel=1e-3))
        K.setup()
        assert K.prob.kernel_name(loop=True) == 'w8::k_mpc_run<16,true,12,4,231,true>', K.prob.kernel_name(loop=True)
        tr = K.run(10, w=0.01 * np.random.default_rng(5).standard_normal((10, B, 12)))
    for i in np.linspace(0, B - 1, 16).astype(int):
        Ko = _oracle(kws[i], 1e-3)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            for k in range(10):
                uo = Ko.output()
                assert np.abs(tr['u'][k, i] - uo).max() <= 1e-7 * max(1e-3, np.abs(uo).max()), (i, k)
                Ko.update(tr['x'][k + 1, i], tr['u'][k, i])
                assert (Ko.res.info.iter, Ko.res.info.status_val) == (tr['iter'][k, i], tr['status'][k, i]), (i, k)


# ---- g. the closed loop's carry on mixed patterns ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [64, 1024])
def test_carry_on_mixed_patterns_headline_kernel(B):
    kws = [rp.ctor(rp.draw(s, 12, 4, 30))[0] for s in range(B)]
    assert rp.kinds_present([rp.draw(s, 12, 4, 30) for s in range(B)]) >= rp.ALL_KINDS
    steps = 12
    w = 0.01 * np.random.default_rng(8).standard_normal((steps, B, 12))
    a, (carried, back, parts) = carry_on_and_off(kws, steps, w=w)
    assert (parts > 0) == (B == 1024), parts                 # (1024 instances: a persistent launch)
    assert (a['status'] == 1).mean() > 0.9
    assert carried > 0, (carried, back)


@pytest.mark.parametrize('tag', ['bcr8', 'bcrt'])
@pytest.mark.parametrize('sid', ['10_3_30', '6_2_20', '12_4_10'])
def test_carry_on_mixed_patterns_generic_kernels(sid, tag):
    """The generic <0,0,MODE_BCRT + 11/21/31> instantiations, 512- and 256-thread workgroups: carry against MPCQP_TUNE_NO_CARRY bit for
    bit (where the round carries at all), and the device loop against the stepwise API bit for bit.  The batches hold Delta-u equality and loose Delta-u rows (the rows
    latw_carry re-types with u_{-1})."""
    from pympc_amd.solver import forced_settings
    nx, nu, Np, _, _ = SHAPES[sid]
    draws = _kws(sid)
    assert {('du', 'eq'), ('du', 'absent')} <= rp.kinds_present(draws)
    kws = [rp.ctor(d)[0] for d in draws]
    steps = 10
    w = 0.01 * np.random.default_rng(9).standard_normal((steps, len(kws), nx))
    K = _dev(draws, tag, 1e-3)
    kn = K.prob.kernel_name(True).replace(' ', '')
    assert kn.split(',')[2:5] == ['0', '0', str(_mode(tag, nx, nu, Np))] and kn.startswith('w8::') == (tag == 'bcr8'), kn
    with forced_settings(backend=tag):
        a, (carried, back, _) = carry_on_and_off(kws, steps, w=w, expect_latency=False)
    # the round carries where it runs the fast termination test (admm_latw: one group of four stages per wave -- every schedule on 512
    # threads, schedule 11 on 256); several groups per wave (schedules 21 and 31 on 256 threads) take the generic check, which never carries
    if tag == 'bcr8' or Np + 1 <= 11:
        assert carried > 0, (carried, back)
    else:
        assert carried == 0, (carried, back)
    K = _dev(draws, tag, 1e-3)
    K2 = _dev(draws, tag, 1e-3)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        tr = K.run(steps, w=w)
        for k in range(steps):
            assert np.array_equal(K2.output(), tr['u'][k]), k
            K2.update(tr['x'][k + 1])
            assert [i.iter for i in K2.prob.infos()] == list(tr['iter'][k]), k


# ---- h. polish ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sid', ['12_4_30', '4_1_20'])
def test_polish_on_mixed_patterns(sid):
    """Equality and loose rows go through the active-set rule of the polish (tests/polish_ref.py) on every instance."""
    K = _dev(_kws(sid), 'auto', 1e-3)
    st = check_against_spec(K.prob)
    assert (st == 1).any(), st
