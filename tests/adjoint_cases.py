"""Named controllers for the adjoint derivatives on the shapes the golden fixtures do not reach (tests/test_adjoint_cases.py pins the
table on the CPU, tests/test_gpu_adjoint_shapes.py holds the device to the restatement on it).

Every instance is  fixtures.random_lti(7100 + seed, nx, nu, Np, xbox=2.0, ubox=0.5, dubox=0.25)  with x0 scaled by the case's factor: tight
boxes, so inequalities are active at the optimum.  Each listed seed ends 'solved' with at least two active inequality rows, no weakly
active row even at 1000 times the device's weak_tol and well-conditioned active rows (tests/test_adjoint_cases.py asserts all of it): a
seed that does not is replaced here, not tolerated there.

Which path of mpcqp_gains a case takes (launch_adjoint, pympc_amd/csrc/mpcqp.hip): the nu unit seeds go four to a solve iff nu > 1,
NB <= 32 and 8 smem_common_doubles(W) <= 160 KiB = 163 840 B, where the work area of W holds at least 4 (m + N NB + 2) doubles -- four row
vectors and four stage-major vectors.  With n = N nx + Nc nu + (soft ? N nx : 0) variables, N = Np + 1, and
m = 2 N nx + Nc nu + (Nc + 1) nu rows (dynamics | state box | input box | Delta-u):
  long200_nu2   N = 201, NB = 16: m = 2 . 804 + 400 + 402 = 2410, N NB + 2 = 3218: 32 (2410 + 3218) = 180 096 B  > 163 840: one seed at a time
  nb32_np60     N = 61,  NB = 32: m = 2 . 1220 + 480 + 488 = 3408, N NB + 2 = 1954: 32 (3408 + 1954) = 171 584 B  > 163 840: one seed at a time
  long100_nu2   N = 101, NB = 16: m = 1210, N NB + 2 = 1618: 90 496 B of columns -- expected to fit with the rest of the block
  long_nu3_held N = 121, NB = 16: m = 1210 + 180 + 183 = 1573, N NB + 2 = 1938: 112 352 B of columns
Both fallback cases are above the limit on the columns alone, whatever the rest of the block needs.  That the others do fit cannot be
read off these numbers alone: the dynamic LDS size of each k_adjoint launch was read from the runtime's launch log (LAB_NOTES.md).
"""
import warnings

import numpy as np

import util
from util import KW, apply_attrs, golden_kwargs, load_golden, stacked, repeated

SEED_BASE = 7100

# The golden fixtures by complementarity at the optimum (tests/test_adjoint_reference.py says what is asserted on which list)
STRICT = ['cart_pole', 'cart_pole_kalman', 'cart_pole_nc1', 'point_mass', 'point_mass_hard', 'point_mass_nc', 'quadcopter_nodu',
          'random_12_4_30', 'random_12_4_30_b', 'random_12_4_30_hard', 'random_20_8_12_hard', 'random_5_3_8', 'random_5_3_8_nc',
          'random_5_3_8_nc_hard', 'small_mimo']
DEGENERATE = ['quadcopter', 'quadcopter_nc', 'accel_brake', 'accel_brake_hard', 'random_20_8_12', 'random_20_8_100']
NO_INEQUALITY_ACTIVE = ['random_12_4_30', 'random_5_3_8_nc', 'cart_pole_kalman']

# name -> nx, nu, Np, Nc, SOFT_ON, x0 scale, seeds, the path it is there for
CASES = {
    'nb16_nu5':       dict(nx=8,  nu=5,  Np=6,   Nc=6,   soft=True,  scale=1.0, seeds=(0, 1, 4),    path='NB 16, column groups 4 + 1'),
    'nb16_nu6':       dict(nx=6,  nu=6,  Np=5,   Nc=5,   soft=True,  scale=1.0, seeds=(0, 1, 4),    path='NB 16, column groups 4 + 2'),
    'nb16_nu7_hard':  dict(nx=7,  nu=7,  Np=4,   Nc=4,   soft=False, scale=1.0, seeds=(0, 1, 2),    path='NB 16, column groups 4 + 3, no slack columns'),
    'nb32_nu5_soft':  dict(nx=20, nu=5,  Np=6,   Nc=6,   soft=True,  scale=1.0, seeds=(6, 7, 9),    path='NB 32 columns with slack variables'),
    'nb32_nu9_held':  dict(nx=18, nu=9,  Np=6,   Nc=3,   soft=True,  scale=1.0, seeds=(1, 4, 5),    path='NB 32 columns, held input (border), groups 4 + 4 + 1'),
    'nb32_nu2':       dict(nx=24, nu=2,  Np=5,   Nc=5,   soft=True,  scale=1.5, seeds=(14, 27),     path='NB 32, one half-empty group'),
    'nb64_nu6':       dict(nx=36, nu=6,  Np=4,   Nc=4,   soft=True,  scale=1.5, seeds=(13, 17, 23), path='NB 64 (wide layout), seeds one at a time'),
    'nb64_nu10_held': dict(nx=30, nu=10, Np=5,   Nc=2,   soft=True,  scale=1.0, seeds=(0, 10),      path='NB 64 with a held input (border)'),
    'nb128_nu5':      dict(nx=64, nu=5,  Np=3,   Nc=3,   soft=True,  scale=1.5, seeds=(7, 1, 2),    path='NB 128 (huge layout)'),
    'long100_nu2':    dict(nx=4,  nu=2,  Np=100, Nc=100, soft=True,  scale=1.0, seeds=(0, 2, 3),    path='grouped-eligible shape in the generic layout, columns fit'),
    'long200_nu2':    dict(nx=4,  nu=2,  Np=200, Nc=200, soft=True,  scale=1.0, seeds=(0, 2),       path='columns do not fit the LDS: seeds one at a time'),
    'long_nu3_held':  dict(nx=5,  nu=3,  Np=120, Nc=60,  soft=True,  scale=1.0, seeds=(2, 3, 7),    path='long, held input, nearly dependent rows (extra sweeps)'),
    'nb32_np60':      dict(nx=20, nu=8,  Np=60,  Nc=60,  soft=True,  scale=1.0, seeds=(19, 20),     path='columns do not fit the LDS at NB 32'),
}
# nb16_nu7_hard with this seed is primal infeasible: the unsolved neighbour of the mixed-status batch (asserted where it is used)
INFEASIBLE = ('nb16_nu7_hard', 11)

FALLBACK = ('long200_nu2', 'nb32_np60')      # nu > 1, NB <= 32, yet one seed at a time
WIDE = ('nb64_nu6', 'nb64_nu10_held', 'nb128_nu5')


def pairs():
    """Every (case, seed) of the table."""
    return [(name, s) for name, c in CASES.items() for s in c['seeds']]


def stage_width(name):
    """NB of the generic layout: the next of 16, 32, 64, 128 at or above nx + nu."""
    c = CASES[name]
    return next(nb for nb in (16, 32, 64, 128) if c['nx'] + c['nu'] <= nb)


def column_bytes(name):
    """Bytes the four columns of a solve need on their own: 8 . 4 (m + N NB + 2)."""
    c = CASES[name]
    N = c['Np'] + 1
    m = 2 * N * c['nx'] + c['Nc'] * c['nu'] + (c['Nc'] + 1) * c['nu']
    return 32 * (m + N * stage_width(name) + 2)


def draw(name, seed):
    """(constructor kwargs of MPCController, attributes to set afterwards) of one instance."""
    from pympc_amd import fixtures
    c = CASES[name]
    kw = dict(fixtures.random_lti(SEED_BASE + seed, nx=c['nx'], nu=c['nu'], Np=c['Np'], xbox=2.0, ubox=0.5, dubox=0.25))
    kw['x0'] = kw['x0'] * c['scale']
    if c['Nc'] != c['Np']:
        kw['Nc'] = c['Nc']
    return kw, ({} if c['soft'] else {'SOFT_ON': False})


def batch_kwargs(name, seeds=None, **settings):
    """BatchMPCController kwargs with the case's seeds (or the given ones) as its instances."""
    c = CASES[name]
    kws = [draw(name, s)[0] for s in (c['seeds'] if seeds is None else seeds)]
    return stacked(kws, Nc=c['Nc'], eps_feas=kws[0]['eps_feas'], SOFT_ON=c['soft'], **settings)


def oracle_controller(name, seed, eps):
    """The instance as an MPCController on the CPU oracle (oracle/osqp_oracle.py), set up and cold-solved at eps_abs = eps_rel = eps."""
    kw, attrs = draw(name, seed)
    return util.oracle_controller(kw, attrs, eps=eps, setup=True, quiet=True, max_iter=4000000)


def oracle_state(K):
    """(P, A, l, u, x, z, y, D, E, c) of an oracle controller's last solve: the argument list of adjoint_ref.adjoint / gains."""
    x, z, y, _ = K.prob.iterate_state()
    D, E, c = K.prob.scaling()
    return (K.P, K.A, np.asarray(K.l, dtype=float), np.asarray(K.u, dtype=float), x, z, y, D, E, c)


def oracle_qp(P, q, A, l, u, eps):
    """The CPU oracle set up on a QP at eps_abs = eps_rel = eps (not solved)."""
    from oracle.osqp_oracle import OSQP
    o = OSQP()
    o.setup(P, q, A, np.clip(l, -1e30, 1e30), np.clip(u, -1e30, 1e30), eps_abs=eps, eps_rel=eps, max_iter=4000000)
    return o


def solve_golden(name, eps):
    """A golden fixture solved by the oracle: (kwargs, QP, result, (x, z, y), (D, E, c))."""
    from polish_ref import golden_qp
    g = load_golden(name)
    P, q, A, l, u = qp = golden_qp(g)
    o = oracle_qp(P, q, A, l, u, eps)
    r = o.solve()
    assert r.info.status == 'solved', (name, r.info.status)
    x, z, y, _ = o.iterate_state()
    return golden_kwargs(g), qp, r, (x, z, y), o.scaling()


# ---- the device under the adjoint tests' settings (tests/test_gpu_adjoint.py, _shapes, _model) ------------------------------------------
EPS = 1e-9
# Every output of mpcqp_adjoint / mpcqp_gains against the restatement, relative to max(1, |.|_inf): the tolerance polishing holds against its
# restatement (tests/test_gpu_polish.py) -- the same factor, the same refinement.  Measured maxima per fixture: LAB_NOTES.md.
TOL = 1e-9
RAW = ('q', 'l', 'u')
CHAINED = ('x0', 'uminus1', 'xref', 'uref')


def controller(kw, eps=EPS, **settings):
    from pympc_amd import MPCController
    attrs = getattr(kw, 'attrs', {})
    kw = KW(kw); kw.attrs = attrs
    kw.update(eps_abs=eps, eps_rel=eps)
    K = apply_attrs(MPCController(**kw), kw)
    K.solver_settings = dict(max_iter=400000, **settings)
    return K


def golden(name):
    return golden_kwargs(load_golden(name))


def solved(kw, **settings):
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        K = controller(kw, **settings); K.setup()
    assert K.res.info.status == 'solved', K.res.info.status
    return K


def device_state(bp, b=0):
    P, q, A, l, u = (v[b] for v in bp.export_qp())
    x, z, y = (v[b] for v in bp.iterate_state())
    D, E, c, _ = bp.scaling()
    return (P, A, l, u, x, z, y, D[b], E[b], c[b])


def random_batch(kws, eps=EPS, **settings):
    """A BatchMPCController (not set up) of instances without a held input at eps, with instance 0's scalar eps_feas."""
    from pympc_amd import BatchMPCController
    return BatchMPCController(**stacked(kws, Nc=None, eps_feas=kws[0]['eps_feas'], eps_abs=eps, eps_rel=eps, max_iter=400000, **settings))


def copies(kw, B, **settings):
    """A BatchMPCController (not set up) of B copies of one instance at EPS, with its scalar eps_feas."""
    from pympc_amd import BatchMPCController
    return BatchMPCController(**repeated(kw, B, eps_feas=kw.get('eps_feas', 1e6), eps_abs=EPS, eps_rel=EPS, max_iter=400000, **settings))


def snapshot(bp):
    x, y, info = bp.solution()
    return [x, y, bytes(info)] + list(bp.iterate_state()) + [np.array(bp.stats()), bp.polish_status()]


def same(a, b):
    return all((p == q) if isinstance(p, bytes) else np.array_equal(p, q, equal_nan=True) for p, q in zip(a, b))


def point_mass_batch(um1_bad=2, B=5, **settings):
    """util.point_mass_batch under the adjoint tests' settings."""
    return util.point_mass_batch(um1_bad, B, eps_abs=EPS, eps_rel=EPS, max_iter=400000, **settings)


def case_batch(name, seeds=None, backend=None):
    """The case's seeds (or the given ones) as a BatchMPCController at EPS, set up and solved, on a forced backend if one is named."""
    from pympc_amd import BatchMPCController
    from pympc_amd.solver import forced_settings
    K = BatchMPCController(**batch_kwargs(name, seeds, eps_abs=EPS, eps_rel=EPS, max_iter=400000))
    with warnings.catch_warnings(), forced_settings(**({'backend': backend} if backend else {})):
        warnings.simplefilter('ignore')
        K.setup()
    return K
