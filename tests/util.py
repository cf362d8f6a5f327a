"""Shared helpers for the test-suite: golden-vector loading, controller construction (single and stacked), error metrics,
backend eligibility by shape and the forced-settings context.  Test modules import helpers from here (or from the case tables and
restatements next to it), never from one another."""
import glob
import json
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_DIR = os.path.join(ROOT, 'tests', 'golden')


def golden_names(prefix='qp_'):
    return sorted(os.path.basename(p)[len(prefix):-4] for p in glob.glob(os.path.join(GOLDEN_DIR, prefix + '*.npz')))


def load_golden(name, prefix='qp_'):
    return np.load(os.path.join(GOLDEN_DIR, '%s%s.npz' % (prefix, name)))


class KW(dict):
    """Constructor kwargs of a fixture; ``attrs`` = hidden switches to set on the controller afterwards (SOFT_ON, mpc.py:233-238)."""
    attrs = {}


def golden_kwargs(g):
    """Constructor kwargs stored in a golden file (keys ``in_*``), attribute switches (keys ``attr_*``) in ``.attrs``."""
    kw = KW()
    for k in g.files:
        if k.startswith('in_'):
            v = g[k]
            kw[k[3:]] = int(v) if k[3:] in ('Np', 'Nc') else (float(v) if v.ndim == 0 else np.array(v))
    kw.attrs = {k[5:]: bool(g[k]) for k in g.files if k.startswith('attr_')}
    return kw


def apply_attrs(K, kw):
    for k, v in getattr(kw, 'attrs', {}).items():
        setattr(K, k, v)
    return K


def golden_csc(g, which):
    return sp.csc_matrix((g[which + '_data'], g[which + '_indices'], g[which + '_indptr']),
                         shape=tuple(g[which + '_shape']))


def update_steps(g):
    steps = []
    s = 0
    while 'upd%d_x' % s in g.files:
        u = g['upd%d_u' % s]
        xr = g['upd%d_xref' % s]
        steps.append(dict(x=g['upd%d_x' % s], u=(u if u.size else None), xref=(xr if xr.size else None),
                          q=g['upd%d_q' % s], l=g['upd%d_l' % s], u_bound=g['upd%d_u_bound' % s]))
        s += 1
    return steps


def kkt_certificate(P, q, A, l, u, x, y):
    """(stationarity, primal violation, complementarity) in the inf-norm, relative to data size."""
    Ax = A @ x
    stat = np.abs(P @ x + q + A.T @ y).max() / max(1.0, np.abs(P @ x).max(), np.abs(q).max(), np.abs(A.T @ y).max())
    pv = max(0.0, (l - Ax).max(), (Ax - u).max()) / max(1.0, np.abs(Ax).max())
    yp, ym = np.maximum(y, 0), np.minimum(y, 0)
    ysc = max(1.0, np.abs(y).max())
    with np.errstate(invalid='ignore'):
        cu = np.where(np.isfinite(u), yp * (u - Ax), np.where(yp > 1e-9 * ysc, np.inf, 0.0)).max()
        cl = np.where(np.isfinite(l), -ym * (Ax - l), np.where(ym < -1e-9 * ysc, np.inf, 0.0)).max()
    return stat, pv, max(cu, cl) / ysc


# ---- closed-loop golden trajectories (tests/golden/make_traj.py) ------------------------------------------------------
def traj_names(output_feedback=False):
    """State-feedback closed loops of pyMPC/mpc.py (default) or the output-feedback ones (traj_kalman_*.npz); the loop of
    the older mpc_no_slack.py class (traj_no_slack_*.npz) has a test of its own."""
    names = sorted(os.path.basename(p)[5:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, 'traj_*.npz')))
    return [n for n in names if n.startswith('kalman_') == output_feedback and not n.startswith('no_slack_')]


def load_traj(name):
    return np.load(os.path.join(GOLDEN_DIR, 'traj_%s.npz' % name), allow_pickle=False)


def cart_pole_plant(x, u, Ts=50e-3):
    """Nonlinear cart-pole + forward Euler, the plant of examples/example_inverted_pendulum.py:10-17,92-103
    (same restatement as in tests/golden/make_traj.py)."""
    M, m, b, ftheta, l, g = 0.5, 0.2, 0.1, 0.1, 0.3, 9.81
    F, v, theta, omega = float(u[0]), x[1], x[2], x[3]
    der = np.zeros(4)
    der[0] = v
    der[1] = (m * l * np.sin(theta) * omega ** 2 - m * g * np.sin(theta) * np.cos(theta) + m * ftheta * np.cos(theta) * omega + F - b * v) / (M + m * (1 - np.cos(theta) ** 2))
    der[2] = omega
    der[3] = ((M + m) * (g * np.sin(theta) - ftheta * omega) - m * l * omega ** 2 * np.sin(theta) * np.cos(theta) - (F - b * v) * np.cos(theta)) / (l * (M + m * (1 - np.cos(theta) ** 2)))
    return x + der * Ts


def closed_loop(K, kw, g, plant, feed_golden_states, tol):
    pattern = str(g['pattern'])
    xs, us = g['x'], g['u']
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        K.setup()
        x, u = np.array(kw['x0'], dtype=float), np.array(kw['uminus1'], dtype=float)
        for k in range(len(us)):
            if pattern == 'update_output':
                K.update(x, u)
                u = K.output()
            else:
                u = K.output()
            scale = max(1e-3, np.abs(us).max())
            assert np.abs(u - us[k]).max() <= tol * scale, (k, u, us[k])
            x = xs[k + 1] if feed_golden_states else plant(x, u)
            assert np.abs(x - xs[k + 1]).max() <= tol * max(1e-3, np.abs(xs).max()), k
            if pattern != 'update_output':
                K.update(x)


def no_slack_loop(K, g, tol):
    """u = K.step(); x+ = Ad x + Bd u; K.update(x)  -- the loop of mpc_no_slack.py:362-371."""
    xs, us = g['x'], g['u']
    K.setup()
    x = xs[0].copy()
    for k in range(len(us)):
        u = K.step()
        assert np.abs(u - us[k]).max() <= tol * max(1e-3, np.abs(us).max()), (k, u, us[k])
        x = K.Ad @ x + K.Bd @ u
        assert np.abs(x - xs[k + 1]).max() <= tol * np.abs(xs).max(), k
        K.update(x)


def no_slack_controller(g):
    from pympc_amd import fixtures
    from pympc_amd.mpc_no_slack import MPCController
    kw = {k: v for k, v in fixtures.point_mass().items() if k != 'eps_feas'}
    kw.update(xmin=g['xmin'], xmax=g['xmax'])
    K = MPCController(**kw)
    K.eps_abs = K.eps_rel = float(g['eps'])          # (the golden run was made at tight tolerance; the class's own is 1e-4)
    K.solver_settings = dict(max_iter=400000)
    return K


# ---- controllers ------------------------------------------------------------------------------------------------------------
def gpu_controller(kw, **settings):
    """An MPCController on the device (not set up) with the fixture's attribute switches and these solver settings."""
    from pympc_amd import MPCController
    K = apply_attrs(MPCController(**kw), kw)
    K.solver_settings = dict(settings)
    return K


def oracle_controller(kw, attrs=None, eps=None, setup=False, solve=True, quiet=False, **settings):
    """An MPCController on the CPU oracle (oracle/osqp_oracle.py).  attrs: switches to set afterwards (None: kw.attrs, util.KW);
    eps: eps_abs = eps_rel = eps over what kw holds; settings: its solver_settings, max_iter included -- every caller passes its own;
    setup: also setup(solve=solve), with warnings ignored if quiet."""
    from pympc_amd import MPCController
    from oracle.osqp_oracle import OSQP
    K = MPCController(**(kw if eps is None else dict(kw, eps_abs=eps, eps_rel=eps)))
    for a, v in (getattr(kw, 'attrs', {}) if attrs is None else attrs).items():
        setattr(K, a, v)
    K.prob = OSQP()
    K.solver_settings = dict(settings)
    if setup:
        with warnings.catch_warnings():
            if quiet:
                warnings.simplefilter('ignore')
            K.setup(solve=solve)
    return K


def controller(kw, oracle=False, **settings):
    """gpu_controller, or oracle_controller with the same arguments."""
    return (oracle_controller if oracle else gpu_controller)(kw, **settings)


class NullProb:
    """Stands in for the solver so that only the host logic runs (like the capture stub)."""
    def __init__(self):
        self.n = None
    def setup(self, P, q, A, l, u, **kw):
        self.n = P.shape[0]
        self.kw = kw
    def update(self, **kw):
        self.last = kw
    def solve(self):
        class R: pass
        r = R(); r.x = np.zeros(self.n); r.info = R(); r.info.status = 'solved'; r.info.obj_val = 0.0
        return r


def held_input_qp(Np, Nc, Qu, QDu, nu=1):
    """pyMPC's QP with a control horizon Nc < Np and input weights that are not dyadic rationals: the stored blocks Qu + 2 QDu and
    (Np - Nc + 1) Qu + QDu (mpc.py:505-526) are rounded sums, so Qu read back from the first one is off by an ulp or two."""
    from pympc_amd import MPCController, fixtures
    kw = fixtures.cart_pole() if nu == 1 else fixtures.random_lti(3, nx=5, nu=nu, Np=Np, xbox=10.0)
    kw.update(Np=Np, Nc=Nc, Qu=Qu * np.eye(nu), QDu=QDu * np.eye(nu))
    K = MPCController(**kw); K.prob = NullProb(); K.setup(solve=False)
    return K


STACKED_KEYS = ('Ad', 'Bd', 'x0', 'xref', 'uref', 'uminus1', 'Qx', 'QxN', 'Qu', 'QDu', 'xmin', 'xmax', 'umin', 'umax', 'Dumin', 'Dumax')


def stacked(kws, **over):
    """BatchMPCController kwargs of a list of single-instance kwargs: every array stacked as float along a new first axis, Np and Nc
    (None if absent) of instance 0, eps_feas per instance as [B, 1] (1e6 where absent).  An instance without uref gets zeros, without
    uminus1 its uref, without QxN its Qx.  ``over`` replaces or adds entries: a caller that passes instance 0's scalar eps_feas, the
    table's Nc, SOFT_ON or solver settings says so here."""
    st = lambda k: np.stack([np.asarray(d[k], dtype=float) for d in kws])
    k0 = kws[0]
    args = {k: st(k) for k in STACKED_KEYS if k in k0 or k not in ('uref', 'uminus1', 'QxN')}
    if 'uref' not in k0:
        args['uref'] = np.zeros((len(kws), np.asarray(k0['Bd']).shape[1]))
    args.setdefault('uminus1', args['uref'])
    args.setdefault('QxN', args['Qx'])
    args.update(Np=k0['Np'], Nc=k0.get('Nc'), eps_feas=np.array([[d.get('eps_feas', 1e6)] for d in kws]))
    args.update(over)
    return args


def repeated(kw, B, **over):
    """stacked() of B copies of one instance."""
    return stacked([kw] * B, **over)


def stacked_batch(kws, **over):
    """A BatchMPCController (not set up) of a list of single-instance kwargs, see stacked()."""
    from pympc_amd import BatchMPCController
    return BatchMPCController(**stacked(kws, **over))


def bench_batch(B, nx, nu, Np, xbox, eps):
    """(BatchMPCController, instance kwargs) of a batch as bench.py builds it: random_lti plants 0 .. B - 1 under shared weights and boxes."""
    from pympc_amd import BatchMPCController, fixtures
    kws = [fixtures.random_lti(i, nx=nx, nu=nu, Np=Np, xbox=xbox) for i in range(B)]
    stack = lambda k: np.stack([np.asarray(kw[k], dtype=float) for kw in kws])
    K = BatchMPCController(stack('Ad'), stack('Bd'), Np=Np, x0=stack('x0'), Qx=np.eye(nx), QxN=np.eye(nx), Qu=0.1 * np.eye(nu), QDu=0.1 * np.eye(nu),
                           xmin=-xbox * np.ones(nx), xmax=xbox * np.ones(nx), umin=-np.ones(nu), umax=np.ones(nu),
                           Dumin=-0.5 * np.ones(nu), Dumax=0.5 * np.ones(nu), eps_feas=1e6, eps_abs=eps, eps_rel=eps)
    return K, kws


def random_case(seed):
    """A seeded random controller: dimensions, horizon split, bound pattern (finite / one-sided / absent), weights
    (including semidefinite ones) and reference shape are all drawn."""
    from pympc_amd import fixtures
    rng = np.random.default_rng(7000 + seed)
    nx = int(rng.integers(1, 14)); nu = int(rng.integers(1, 6))
    Np = int(rng.integers(2, 26)); Nc = int(rng.integers(1, Np + 1)) if rng.random() < 0.5 else Np
    kw = dict(fixtures.random_lti(9000 + seed, nx=nx, nu=nu, Np=Np, xbox=4.0))
    kw['x0'] = 0.5 * kw['x0']
    if Nc != Np:
        kw['Nc'] = Nc
    inf = np.inf
    def pattern(lo, hi):
        lo, hi = lo.copy(), hi.copy()
        for i in range(lo.size):
            t = rng.random()
            if t < 0.2: lo[i] = -inf
            elif t < 0.4: hi[i] = inf
            elif t < 0.5: lo[i], hi[i] = -inf, inf
        return lo, hi
    kw['xmin'], kw['xmax'] = pattern(kw['xmin'], kw['xmax'])
    kw['Dumin'], kw['Dumax'] = pattern(kw['Dumin'], kw['Dumax'])
    if rng.random() < 0.3:
        kw['umin'], kw['umax'] = pattern(kw['umin'], kw['umax'])
    w = rng.random()
    if w < 0.25: kw['QDu'] = np.zeros((nu, nu))                       # Qu > 0 keeps the optimum unique
    elif w < 0.5: kw['Qu'] = np.zeros((nu, nu))                       # QDu > 0 does
    G = rng.standard_normal((nx, nx)); kw['Qx'] = G @ G.T / nx        # dense PSD state weight
    if rng.random() < 0.5: kw['QxN'] = 3.0 * kw['Qx']
    if rng.random() < 0.3: kw['xref'] = 0.2 * rng.standard_normal((Np + 1, nx))
    else: kw['xref'] = 0.2 * rng.standard_normal(nx)
    kw['uref'] = 0.1 * rng.standard_normal(nu)
    kw['uminus1'] = 0.1 * rng.standard_normal(nu)
    kw['eps_feas'] = float(10.0 ** rng.integers(2, 7))
    return kw


def point_mass_batch(um1_bad=2, B=5, **settings):
    """(BatchMPCController, instance kwargs) of B point masses (not set up), x0 scaled 0.6 .. 1, instance um1_bad infeasible; settings: eps_abs,
    eps_rel, max_iter and the like."""
    from pympc_amd import BatchMPCController, fixtures
    kw = fixtures.point_mass()
    st = lambda a: np.stack([np.asarray(a, dtype=float)] * B)
    um1 = st(kw['uminus1'] if 'uminus1' in kw else np.zeros(1))
    um1[um1_bad] = 5.0                               # tests/test_gpu_parity.py's infeasible recipe for one instance
    x0 = st(kw['x0']) * np.linspace(0.6, 1.0, B)[:, None]
    K = BatchMPCController(**repeated(kw, B, Nc=None, x0=x0, uminus1=um1, eps_feas=kw.get('eps_feas', 1e6), **settings))
    return K, kw


def complete(kw):
    """Fixture dict with every optional controller argument spelled out (what the stacked constructor wants)."""
    kw = dict(kw)
    nx, nu = kw['Ad'].shape[0], kw['Bd'].shape[1]
    kw.setdefault('uref', np.zeros(nu)); kw.setdefault('xref', np.zeros(nx)); kw.setdefault('uminus1', kw['uref'])
    kw.setdefault('QxN', kw['Qx'])
    return kw


def info_tuple(infos):
    return np.array([(i.status, i.iter, i.rho_updates, i.obj_val, i.pri_res, i.dua_res, i.rho) for i in infos], dtype=float)


# ---- error metrics ----------------------------------------------------------------------------------------------------------
def rel(a, b):
    """max |a - b| divided by max |b| (floored at 1e-300): purely relative."""
    return np.abs(a - b).max() / max(1e-300, np.abs(b).max())


def rel1(a, b):
    """max |a - b| divided by max(1, max |b|): relative for large b, absolute for small."""
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def rel1_any(a, b):
    """rel1 of anything array-like, as a float; 0 for empty arrays."""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return float(np.abs(a - b).max() / max(1.0, np.abs(b).max())) if b.size else 0.0


# ---- which KKT backends a shape is eligible for (mpcqp_create's rules) --------------------------------------------------------
def shape_of(kw):
    """(nx, nu, Np, Nc) of controller kwargs; Nc None where it is not given."""
    nx, nu = np.atleast_2d(kw['Bd']).shape if np.ndim(kw['Bd']) == 2 else (np.asarray(kw['Ad']).shape[0], 1)
    return nx, nu, kw['Np'], kw.get('Nc')


def dense_eligible(nx, nu, Np, Nc=None):
    """The dense register-resident inverse: N (nx + nu) <= 128 and no held input."""
    return (Np + 1) * (nx + nu) <= 128 and Nc in (None, Np)


def bcr_schedule(nx, nu, Np, Nc=None):
    """Stage count of the cyclic-reduction schedule mpcqp_create gives the shape (11, 21 or 31 >= Np + 1), or 0: 16 x 16 stages,
    no held input, at most 31 stages."""
    if nx + nu > 16 or Nc not in (None, Np) or Np + 1 > 31:
        return 0
    return 11 if Np + 1 <= 11 else 21 if Np + 1 <= 21 else 31


def eligible_backends(nx, nu, Np, Nc=None):
    out = ['sweeps']
    if dense_eligible(nx, nu, Np, Nc):
        out.append('dense')
    if bcr_schedule(nx, nu, Np, Nc):
        out += ['bcr', 'bcr8', 'bcrt']
    return out


def golden_shape(name):
    return shape_of(golden_kwargs(load_golden(name)))


def golden_dense_eligible(name):
    return dense_eligible(*golden_shape(name))


def golden_bcr_schedule(name):
    return bcr_schedule(*golden_shape(name))


def golden_backends(name):
    """Every backend the golden fixture may be forced to."""
    return eligible_backends(*golden_shape(name))


def forced(backend=None, **more):
    """Every controller built inside the block gets these mpcqp_settings fields (pympc_amd.solver.forced_settings): the KKT backend
    (include/mpcqp.h: enum mpcqp_backend; None: what mpcqp_create picks), tuning=..., and so on."""
    from pympc_amd.solver import forced_settings
    return forced_settings(**(more if backend is None else dict(more, backend=backend)))


def carry_on_and_off(kws, steps, nruns=1, w=None, expect_latency=True, run_kw=None, **kw):
    """The same closed loop with and without the carry: every array it produces must agree, and so must the launch structure (queue-item parts
    of a persistent launch).  Returns the arrays and the carry counters (carried, handed back, parts) of the run with the carry."""
    from pympc_amd import _lib
    from pympc_amd.solver import forced_settings
    out, cs = [], []
    for tuning in (0, _lib.TUNE_NO_CARRY):
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            with forced_settings(tuning=tuning):          # (the handle, and with it its settings, is made by setup())
                K = stacked_batch(kws, **kw)
                K.setup()
            if expect_latency:
                assert '231' in K.prob.kernel_name(True).replace(' ', ''), K.prob.kernel_name(True)
            res = []
            for i in range(nruns):
                rk = dict(run_kw(i)) if run_kw else {}
                if w is not None:
                    rk['w'] = w[steps * i:steps * (i + 1)]
                res.append(K.run(steps, **rk))
        arrs = {k: np.concatenate([r[k] for r in res]) for k in res[0]}
        x, y, _ = K.prob.solution()
        arrs['sol_x'], arrs['sol_y'] = x, y
        arrs['info'] = info_tuple(K.prob.infos())
        arrs['output'] = K.output()
        out.append(arrs)
        cs.append(K.prob.carry_stats())
    a, b = out
    assert sorted(a) == sorted(b), (sorted(a), sorted(b))
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    assert cs[1][:2] == (0, 0), cs                        # (MPCQP_TUNE_NO_CARRY: the round never carries)
    assert cs[0][2] == cs[1][2], cs                       # (... and the launch is cut into the same parts)
    return a, cs[0]


# ---- shapes of the grouped and wide layouts (tests/test_gpu_group.py, tests/test_gpu_wide.py, tests/settings_cases.py) ------------
def group_kw(shape, seed=0, **more):
    """Controller kwargs of a grouped-stage shape (nx, nu, Np, Nc, soft) of tests/test_gpu_group.py."""
    from pympc_amd import fixtures
    nx, nu, Np, Nc, soft = shape
    if (nx, nu) == (4, 1):
        kw = dict(fixtures.cart_pole()); kw.update(Np=Np)                  # the notebook's plant (unstable: what makes long horizons hard)
    else:
        kw = dict(fixtures.random_lti(71000 + 13 * nx + nu + seed, nx=nx, nu=nu, Np=Np, xbox=4.0))
        kw['x0'] = 0.4 * kw['x0']
    kw.update(Nc=Nc)
    kw.update(more)
    return kw


# (nx, nu, Np, Nc) by tag
WIDE = {'33': (25, 8, 3, 3), '48': (40, 8, 10, 10), '40_nc': (30, 10, 12, 5), '64': (56, 8, 5, 5), '64_u': (48, 16, 4, 4), '36_long': (32, 4, 40, 40),
        # 64 < nx + nu <= 128 (pympc_amd/csrc/mpcqp_huge.h: the merely-correct backend of round 4; VERDICT r3 asked for (70,10,5) and (100,20,3))
        '80': (70, 10, 5, 5), '120': (100, 20, 3, 3), '68_nc': (60, 8, 6, 2), '128': (96, 32, 2, 2),
        # a held input (Nc < Np) with MANY inputs: border_factor's Sigma and Sigma^-1 (2 nu^2 doubles) used to run past the LDS work area of the
        # 128-wide backend (3 200 doubles needed, 1 464 there) and the generic border_pre wrote 2 nu doubles into 128 (round-4 advisor finding)
        '70_nc_nu40': (30, 40, 3, 2), '90_nc_nu70': (20, 70, 3, 2), '56_nc_nu24': (32, 24, 4, 2)}


def wide_kw(tag):
    """Controller kwargs of a wide-stage shape of WIDE."""
    from pympc_amd import fixtures
    nx, nu, Np, Nc = WIDE[tag]
    kw = dict(fixtures.random_lti(1200 + nx * 7 + nu, nx=nx, nu=nu, Np=Np, xbox=3.0))
    kw['x0'] = 0.3 * kw['x0']
    if Nc != Np:
        kw['Nc'] = Nc
    return kw


# ---- the compiler's resource remarks of the build ----------------------------------------------------------------------------
KERNEL_RESOURCES = os.path.join(ROOT, 'pympc_amd', 'libmpcqp_hip.kernel_resources.txt')


def kernel_resources():
    """{kernel: {remark: value}} of the compiler's resource remarks of the build (pympc_amd/libmpcqp_hip.kernel_resources.txt)."""
    import pytest
    if not os.path.exists(KERNEL_RESOURCES):
        pytest.skip('no kernel_resources.txt next to the library (built without csrc/build.sh)')
    out, cur = {}, None
    for line in open(KERNEL_RESOURCES):
        m = re.match(r'\s*Function Name: (\S+)', line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.match(r'\s*([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+)', line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return out


# ---- bench.py in a child process -----------------------------------------------------------------------------------------------
def run_bench(env, *flags):
    """bench.py with this environment and these flags, 280 s at the most: it must exit with 0 and print exactly ONE JSON line, the LAST line
    of its stdout (what the driver parses; a collective library's banner must not land behind it).  Returns the line, parsed."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + list(flags), env=env, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
    assert len(lines) == 1, r.stdout
    assert r.stdout.rstrip().splitlines()[-1] == lines[0], r.stdout[-1500:]
    return json.loads(lines[0])
