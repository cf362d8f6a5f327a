"""The table of tests/rollout_est_cases.py pinned on the CPU oracle, the recursion of tests/rollout_est_ref.py (include/mpcqp_rollout_est.h)
against central differences of the stepped output-feedback loop on the oracle, and the new struct of pympc_amd._lib against a C program
compiled from the header.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rollout_cases as rc
import rollout_est_cases as ec
import rollout_est_ref as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_tapes = {}


def _rollout(name, seed):
    """The oracle's K + 1 solves of one (case, seed) under output feedback, made once."""
    if (name, seed) not in _tapes:
        kw, attrs = rc.draw(name, seed)
        e = ec.estimator(name, seed)
        tape, X, XH, Y, U, scaling = ec.oracle_rollout(kw, attrs, rc.CASES[name]['K'], e['C'], e['L'], e['x_true0'], v=e['v'], w=e['w'], with_last=True)
        _tapes[(name, seed)] = (kw, attrs, tape, scaling)
    return _tapes[(name, seed)]


def test_the_table_covers_the_cases_of_the_state_feedback_rollout():
    assert set(ec.SEEDS) == {n for n, c in rc.CASES.items() if not c['tv']}
    assert ec.SEEDS['first'] == (0, 3, 4, 6) and 5 not in ec.SEEDS['first']
    for name, seeds in ec.SEEDS.items():
        assert len(seeds) >= 2 and max(seeds) < 100, name
        assert ec.ny_of(name) == (2 if rc.CASES[name]['nx'] < 12 else 3)


@pytest.mark.parametrize('name,seed', ec.pairs())
def test_every_listed_seed_meets_the_conditions(name, seed):
    kw, attrs, tape, scaling = _rollout(name, seed)
    f = rc.tape_facts(kw, attrs, tape, scaling)
    print('ROLLOUT_EST_CASE %s/%d: n_ineq %s n_weak %s same %s' % (name, seed, f['n_ineq'].tolist(), f['n_weak'].tolist(), f['same'].astype(int).tolist()))
    assert f['solved'].all(), (name, seed, f['solved'])
    assert (f['n_weak'] == 0).all(), (name, seed, f['n_weak'])
    assert f['n_ineq'].max() >= 2, (name, seed, f['n_ineq'])
    assert f['same'].any() and not f['same'].all(), (name, seed, f['same'])


def test_the_reuse_instance_takes_three_factorizations_over_six_entries():
    K = rc.CASES[ec.FIRST]['K']
    kw, attrs, tape, scaling = _rollout(ec.FIRST, ec.REUSE_SEED)
    same = rc.tape_facts(kw, attrs, tape[:K], scaling)['same']
    assert same.astype(int).tolist() == [0, 0, 1, 1, 1]
    assert 1 < 1 + int(np.count_nonzero(~same)) < K


# ---- the recursion against central differences of the stepped loop ---------------------------------------------------------------------
FD_SEEDS = (0, 3)
H = 1e-6
EPS_FD = 1e-10


@pytest.mark.parametrize('own_plant', (False, True), ids=('plant_is_model', 'plant_given'))
@pytest.mark.parametrize('seed', FD_SEEDS)
def test_the_restatement_against_central_differences(seed, own_plant):
    """L = sum <Gx[k], x_k> + <Gxh[k], xh_k> + <Gu[k], u_k> + <Gy[k], y_k> of the stepped output-feedback loop: rollout_est_ref against
    (L(p + h) - L(p - h)) / 2h in entries of xh_0, x_0, L, C, v[k], w[k], u_{-1}, uref, Ad, Bd, within 1e-4 max(1, |fd|_inf)."""
    c = rc.CASES[ec.FIRST]
    K, nx, nu, ny = c['K'], c['nx'], c['nu'], ec.ny_of(ec.FIRST)
    kw, attrs = rc.draw(ec.FIRST, seed)
    kw = er.adjoint_model_ref.full_kwargs(kw)
    est = ec.estimator(ec.FIRST, seed)
    rng = np.random.default_rng(60 + seed)
    Gx, Gxh, Gu, Gy = rng.standard_normal((K + 1, nx)), rng.standard_normal((K + 1, nx)), rng.standard_normal((K, nu)), rng.standard_normal((K, ny))
    Ap = Bp = None
    if own_plant:                                          # (a draw of its own: it keeps every row of both seeds 1e-3 away from a kink, asserted below)
        prng = np.random.default_rng(160 + seed)
        Ap = kw['Ad'] + 0.02 * prng.standard_normal((nx, nx)); Bp = kw['Bd'] + 0.02 * prng.standard_normal((nx, nu))
    par = dict(C=est['C'], L=est['L'], x_true0=est['x_true0'], v=est['v'], w=est['w'], Ap=Ap, Bp=Bp)

    def run(k2, q):
        return ec.oracle_rollout(k2, attrs, K, q['C'], q['L'], q['x_true0'], v=q['v'], w=q['w'], Ap=q['Ap'], Bp=q['Bp'], eps=EPS_FD)

    tape, X, XH, Y, U, (D, E, cs) = run(kw, par)
    f = rc.tape_facts(kw, attrs, tape, (D, E, cs))
    assert f['solved'].all() and (f['n_weak'] == 0).all(), (f['solved'], f['n_weak'])      # (nothing excluded: no kink on the way)
    ref = er.sweep(kw, attrs, tape, D, E, cs, par['C'], par['L'], G_x=Gx, G_xh=Gxh, G_u=Gu, G_y=Gy, Ap=Ap, Bp=Bp)
    assert ref['n_solved'] == K and (ref['status'] == 1).all()

    def fd(change):
        vals = []
        for sgn in (1.0, -1.0):
            k2 = {k: (np.array(v, dtype=float) if isinstance(v, np.ndarray) else v) for k, v in kw.items()}
            q = {k: (None if v is None else np.array(v, dtype=float)) for k, v in par.items()}
            change(k2, q, sgn * H)
            _, X2, XH2, Y2, U2, _ = run(k2, q)
            vals.append(float((Gx * X2).sum() + (Gxh * XH2).sum() + (Gu * U2).sum() + (Gy * Y2).sum()))
        return (vals[0] - vals[1]) / (2 * H)

    def bump(where, key, idx):
        def change(k2, q, h):
            a = (k2 if where == 'kw' else q)[key]
            a[idx] += h
        return change

    checks = []
    for j in (0, nx - 1):
        checks.append(('xh0[%d]' % j, ref['eta'][0][j], fd(bump('kw', 'x0', j))))
        checks.append(('x0[%d]' % j, ref['lam'][0][j], fd(bump('par', 'x_true0', j))))
    for idx in ((0, 0), (nx - 1, ny - 1), (1, 1)):
        checks.append(('L[%d,%d]' % idx, ref['L'][idx], fd(bump('par', 'L', idx))))
    for idx in ((0, 0), (ny - 1, nx - 1), (1, 2)):
        checks.append(('C[%d,%d]' % idx, ref['C'][idx], fd(bump('par', 'C', idx))))
    for idx in ((0, 1), (K - 2, 0)):
        checks.append(('v[%d][%d]' % idx, ref['v'][idx], fd(bump('par', 'v', idx))))
    for idx in ((0, 1), (K - 2, 3)):
        checks.append(('w[%d][%d]' % idx, ref['lam'][idx[0] + 1][idx[1]], fd(bump('par', 'w', idx))))
    for j in range(nu):
        checks.append(('um1[%d]' % j, ref['uminus1'][j], fd(bump('kw', 'uminus1', j))))
        checks.append(('uref[%d]' % j, ref['uref'][j], fd(bump('kw', 'uref', j))))
    for idx in ((0, 0), (1, 2), (3, 1)):
        # the controller's Ad is the estimator's too, and with the plant equal to the model the plant's: d_Ad + d_Ae (+ d_Ap)
        want = ref['Ad'][idx] + ref['Ae'][idx] + (ref['Ap'][idx] if not own_plant else 0.0)
        checks.append(('Ad[%d,%d]' % idx, want, fd(bump('kw', 'Ad', idx))))
    for idx in ((0, 1), (2, 0)):
        want = ref['Bd'][idx] + ref['Be'][idx] + (ref['Bp'][idx] if not own_plant else 0.0)
        checks.append(('Bd[%d,%d]' % idx, want, fd(bump('kw', 'Bd', idx))))
    if own_plant:
        checks.append(('Ap[1,1]', ref['Ap'][1, 1], fd(bump('par', 'Ap', (1, 1)))))
        checks.append(('Bp[2,1]', ref['Bp'][2, 1], fd(bump('par', 'Bp', (2, 1)))))
    scale = max(1.0, max(abs(v) for _, _, v in checks))
    for name, got, want in checks:
        print('ROLLOUT_EST_FD seed %d %s %s: ref %+.6e fd %+.6e' % (seed, 'own plant' if own_plant else 'model', name, got, want))
    for name, got, want in checks:
        assert abs(got - want) <= 1e-4 * scale, (name, got, want)
    assert max(abs(v) for _, _, v in checks) > 1e-3        # (the differences are not all in the noise)


# ---- the binding ----------------------------------------------------------------------------------------------------------------------
FUNCTIONS = ['mpcqp_rollout_adjoint_est', 'mpcqp_rollout_est', 'mpcqp_rollout_est_tape_bytes', 'mpcqp_rollout_get_tape_est']
FIELDS = ['struct_size', 'G_xhat', 'G_y', 'eta', 'd_C', 'd_L', 'd_v', 'd_Ae', 'd_Be']


def test_the_struct_is_the_one_a_c_compiler_lays_out(tmp_path):
    from pympc_amd import _lib
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mpcqp_rollout_est.h"\nint main(void) {\n'
                   '  printf("sizeof %zu\\n", sizeof(mpcqp_rollout_est_io));\n'
                   + ''.join('  printf("%s %%zu\\n", offsetof(mpcqp_rollout_est_io, %s));\n' % (f, f) for f in FIELDS) + '  return 0;\n}\n')
    exe = tmp_path / 'layout'
    subprocess.check_call([os.environ.get('CC', 'cc'), '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert [n for n, _ in _lib.RolloutEstIO._fields_] == FIELDS
    assert C.sizeof(_lib.RolloutEstIO) == int(out['sizeof']) == 8 + 8 * 8
    for f in FIELDS:
        assert getattr(_lib.RolloutEstIO, f).offset == int(out[f]), f


def test_the_functions_are_the_headers_and_a_library_without_them_is_refused():
    from pympc_amd import _lib
    from abi import header, header_functions
    assert header_functions(header('mpcqp_rollout_est.h')) == sorted(_lib.ROLLOUT_EST_SYMBOLS) == FUNCTIONS
    assert not set(FUNCTIONS) & set(_lib.SYMBOLS + _lib.ROLLOUT_SYMBOLS + _lib.ADJOINT_SYMBOLS + _lib.ADJOINT_MODEL_SYMBOLS + _lib.MODEL_SYMBOLS + _lib.POLISH_SYMBOLS)

    class Without:                                         # a library that exports none of them
        pass
    assert not _lib.has_rollout_est(Without())
    from pympc_amd.solver import BatchProblem
    p = BatchProblem.__new__(BatchProblem)
    p._L = Without()
    with pytest.raises(NotImplementedError, match=r'include/mpcqp_rollout_est\.h'):
        p._need('rollout_est')
