"""The mixed row-pattern generator (tests/row_patterns.py) and, on the CPU twin of the C ABI (oracle/libmpcqp_cpu.so), the host path of
the GPU tests in tests/test_gpu_row_types.py: a batch whose instances mix every row type, then changes of row types through the raw seam
(BatchProblem.update_vectors), instance by instance against the oracle."""
import warnings

import numpy as np
import pytest

import row_patterns as rp
from abi import twin  # noqa: F401  (fixture)

# the pinned shapes of tests/test_gpu_row_types.py: (nx, nu, Np, Nc, soft)
SHAPES = [(12, 4, 30, None, True), (10, 3, 30, None, True), (6, 2, 20, None, True), (12, 4, 10, None, True), (3, 1, 30, None, True),
          (4, 1, 20, None, True), (20, 8, 12, None, True), (18, 6, 12, None, True), (30, 10, 8, None, True), (60, 20, 4, None, True),
          (3, 1, 200, None, True), (4, 1, 150, 75, True), (12, 4, 30, 10, True), (12, 4, 30, None, False)]
IDS = ['%d_%d_%d%s%s' % (nx, nu, Np, '_nc%d' % Nc if Nc else '', '' if soft else '_hard') for nx, nu, Np, Nc, soft in SHAPES]


def _model(kw):
    nx, nu = kw['Bd'].shape
    return dict(nx=nx, nu=nu, Np=kw['Np'], Nc=kw.get('Nc', kw['Np']))


def test_draw_is_deterministic():
    for sh in SHAPES[:4]:
        a, b = rp.draw(5, *sh[:4], soft=sh[4]), rp.draw(5, *sh[:4], soft=sh[4])
        assert sorted(a) == sorted(b)
        for k in a:
            if isinstance(a[k], np.ndarray):
                assert np.array_equal(a[k], b[k]), k
            else:
                assert a[k] == b[k], k
        assert not np.array_equal(rp.draw(6, *sh[:4], soft=sh[4])['Ad'], a['Ad'])
        r1, r2 = np.random.default_rng(1), np.random.default_rng(1)
        f1, f2 = rp.flip_types(a, r1), rp.flip_types(b, r2)
        assert f1[0]['_flipped'] == f2[0]['_flipped'] and np.array_equal(f1[1], f2[1]) and np.array_equal(f1[2], f2[2])


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_pinned_batches_hold_every_row_kind(shape):
    """Every batch of 8 the GPU tests run holds every kind of every class, at least one instance's row types differ from instance 0's,
    the vectors have the reference's stage-periodic structure, and the draw's feasibility rules hold."""
    from pympc_amd import qp_recover
    nx, nu, Np, Nc, soft = shape
    kws = rp.batch(nx, nu, Np, Nc, soft)
    assert len(kws) == 8 and len(set(rp.batch_seeds(nx, nu, Np, Nc, soft))) == 8
    assert rp.kinds_present(kws) >= rp.ALL_KINDS
    t0 = rp.row_types(kws[0])
    assert any(not np.array_equal(rp.row_types(kw), t0) for kw in kws[1:])
    assert {-1, 0, 1} <= set(np.concatenate([rp.row_types(kw)[(Np + 1) * nx:] for kw in kws]))        # (beyond the dynamics rows)
    for kw in kws:
        l, u = rp.bounds(kw)
        qp_recover.check_vectors(_model(kw), l, u)
        c = kw['uminus1'][0]
        assert np.all(kw['uminus1'] == c) and np.all(kw['umin'] <= c) and np.all(c <= kw['umax'])
        assert np.all(kw['Dumin'] <= 0) and np.all(0 <= kw['Dumax']) and kw['Dumin'][-1] <= -c <= kw['Dumax'][-1]
        assert not (np.all(kw['Qu'] == 0) and np.all(kw['QDu'] == 0))
        if not soft:
            fin = np.isfinite(kw['xmin']) | np.isfinite(kw['xmax'])
            assert np.all(np.minimum(kw['x0'] - kw['xmin'], kw['xmax'] - kw['x0'])[fin] > 2.0)
    rng = np.random.default_rng(0)
    kw = kws[0]
    for _ in range(6):
        new, l, u = rp.flip_types(kw, rng)
        qp_recover.check_vectors(_model(kw), l, u)
        cls, j, kind = new['_flipped']
        assert new['_kinds'][cls][j] == kind != kw['_kinds'][cls][j]
        assert np.array_equal(l[:nx], u[:nx]) and np.array_equal(l[:nx], -kw['x0'])
        assert not np.array_equal(rp.row_types(new), rp.row_types(kw))
        kw = new


@pytest.mark.parametrize('shape', [SHAPES[0], SHAPES[4], SHAPES[11], SHAPES[13]], ids=[IDS[0], IDS[4], IDS[11], IDS[13]])
def test_mixed_batch_and_type_changes_through_the_twin(twin, shape):  # noqa: F811
    """The mixed batch on the twin, then three successive flip_types updates of every instance through update_vectors, against the oracle
    updated with the same vectors: status equal, u* within 1e-6 at eps 1e-9."""
    from pympc_amd import BatchMPCController
    nx, nu, Np, Nc, soft = shape
    kws = rp.batch(nx, nu, Np, Nc, soft)
    n_x, n_u = (Np + 1) * nx, (Nc or Np) * nu
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        K = BatchMPCController(**rp.stack(kws, eps_abs=1e-9, eps_rel=1e-9, max_iter=400000))
        K.setup()
        Ko = [rp.oracle(kw, 1e-9) for kw in kws]
        rngs = [np.random.default_rng(100 + b) for b in range(len(kws))]
        cur = list(kws)
        for step in range(4):
            x, _, info = K.prob.solution()
            for b, ko in enumerate(Ko):
                assert K.prob.status_string(info[b].status) == ko.res.info.status, (step, b)
                uo = ko.res.x[n_x:n_x + n_u]
                assert np.abs(x[b][n_x:n_x + n_u] - uo).max() <= 1e-6 * max(1e-3, np.abs(uo).max()), (step, b)
            if step == 3:
                break
            L, U = [], []
            for b in range(len(kws)):
                cur[b], l, u = rp.flip_types(cur[b], rngs[b])
                L.append(l), U.append(u)
                Ko[b].prob.update(l=l, u=u)
                Ko[b].res = Ko[b].prob.solve()
            K.prob.update_vectors(None, np.stack(L), np.stack(U))
            K.prob.solve_async()
    assert sum(i.status == 1 for i in K.prob.infos()) >= 7
