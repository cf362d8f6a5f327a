"""Non-default OSQP settings for the device solver (tests/test_settings_cases.py pins the table on the CPU oracle, tests/test_gpu_settings.py
holds the kernels to the oracle on it).

A (case, setting) pair is listed only if the oracle's (status, iter, rho_updates) is the same at eps_abs = eps_rel = 1e-3 and at 0.97 and 1.03
times that, and the same again when the oracle eliminates its KKT matrix in the natural order instead of the minimum-degree one (two roundings of
one algorithm): a rounding-level difference on the device then cannot move a count.  The same holds for every step of a listed closed loop.
(What the second half is there for: with check_termination = 0 an easy problem sits at its optimum long before iteration 400, both residuals
are rounding noise of 1e-13 .. 1e-15, and so is the rho estimate made from their ratio every 100 iterations -- the oracle's two orders disagree on
rho_updates for three such pairs.)  A pair
that moves is written down in MOVES, not tolerated, and so is one on which the setting cannot be told from the defaults (SAME_AS_DEFAULT: a test
of it would pass on a kernel that ignored the setting).  Where that costs a kernel family a setting, another instance of the family's shape
carries it: the *_tight instances and random_20_8_12_b, random_lti draws with a unit state box, which take a few hundred iterations and several
rho updates and are listed for all fifteen settings (random_12_4_30_tight: all but chk0).  tests/test_settings_cases.py asserts all of it.
"""
import warnings

import numpy as np

EPS = 1e-3
BAND = (1.0, 0.97, 1.03)          # the tolerances a listed pair's counts must not depend on, as factors on EPS

# name -> the settings, and the path through the stop schedule / the iteration / the factor the setting is there for
SETTINGS = {
    'chk1':        (dict(check_termination=1), 'rounds of one iteration'),
    'chk7':        (dict(check_termination=7), 'a round length that is not 25'),
    'chk10_rho15': (dict(check_termination=10, adaptive_rho_interval=15), 'stops that are a rho estimate only, between the checks'),
    'rho30':       (dict(adaptive_rho_interval=30), 'rho-only stops at the default round length'),
    'alpha1':      (dict(alpha=1.0), 'no relaxation'),
    'alpha1.8':    (dict(alpha=1.8), 'relaxation above the default'),
    'sigma1e-2':   (dict(sigma=1e-2), 'the regularisation of the KKT matrix'),
    'rho1':        (dict(rho=1.0), 'the initial step size'),
    'scaling0':    (dict(scaling=0), 'no equilibration: D = E = c = 1'),
    'scaling3':    (dict(scaling=3), 'three Ruiz passes'),
    'noadapt':     (dict(adaptive_rho=0, max_iter=1000), 'no rho adaptation'),
    'tol1.5':      (dict(adaptive_rho_tolerance=1.5, adaptive_rho_interval=25), 'many refactorizations'),
    'chk0':        (dict(check_termination=0, max_iter=400), 'no test until the end'),
    'max60':       (dict(max_iter=60), 'a limit that is not a multiple of the round'),
    'max40':       (dict(max_iter=40), 'a limit that is not a multiple of the round'),
}
ITERATION_SETTINGS = ('alpha1', 'alpha1.8', 'sigma1e-2', 'rho1', 'scaling0', 'scaling3')      # what changes the iteration or the factor

# kernel families with an ADMM body or a check of their own
FAMILIES = ('dense', 'bcr11', 'bcr31', 'nb32', 'border', 'grouped', 'wide64', 'wide128')

# name -> family, how the instance is made (golden: tests/golden/qp_<name>.npz; group / wide: util.group_kw and util.wide_kw, the builders of
# tests/test_gpu_group.py and tests/test_gpu_wide.py; lti: fixtures.random_lti), the backends it is forced on (None: what mpcqp_create picks)
CASES = {
    'point_mass':          dict(family='dense',   make=('golden', 'point_mass'), backends=('dense',)),
    'cart_pole':           dict(family='dense',   make=('golden', 'cart_pole'), backends=('dense',)),
    'cart_pole_bcr':       dict(family='bcr11',   make=('golden', 'cart_pole'), backends=('bcr', 'bcr8', 'bcrt')),
    'random_5_3_8':        dict(family='bcr11',   make=('golden', 'random_5_3_8'), backends=('bcr', 'bcr8', 'bcrt')),
    'quadcopter':          dict(family='bcr11',   make=('golden', 'quadcopter'), backends=('bcr8',)),
    'random_12_4_30':      dict(family='bcr31',   make=('golden', 'random_12_4_30'), backends=('bcr', 'bcr8', 'bcrt', 'sweeps')),
    'random_12_4_30_hard': dict(family='bcr31',   make=('golden', 'random_12_4_30_hard'), backends=('bcr', 'bcr8', 'bcrt', 'sweeps')),
    'random_12_4_30_tight': dict(family='bcr31',  make=('lti', dict(index=24, nx=12, nu=4, Np=30, xbox=1.0)), backends=('bcr8', 'sweeps')),
    'random_20_8_12':      dict(family='nb32',    make=('golden', 'random_20_8_12'), backends=(None,)),
    'random_20_8_12_b':    dict(family='nb32',    make=('lti', dict(index=22, nx=20, nu=8, Np=12, xbox=1.0)), backends=(None,)),
    'random_5_3_8_nc':     dict(family='border',  make=('golden', 'random_5_3_8_nc'), backends=('sweeps',)),
    'cart_pole_nc1':       dict(family='border',  make=('golden', 'cart_pole_nc1'), backends=('sweeps',)),
    'group_3_2_50_20':     dict(family='grouped', make=('group', (3, 2, 50, 20, True)), backends=(None,)),
    'group_5_3_40_40':     dict(family='grouped', make=('group', (5, 3, 40, 40, True)), backends=(None,)),
    'group_3_2_50_20_tight': dict(family='grouped', make=('lti', dict(index=25, nx=3, nu=2, Np=50, Nc=20, xbox=1.0)), backends=(None,)),
    'wide_25_8_3':         dict(family='wide64',  make=('wide', '33'), backends=(None,)),
    'wide_25_8_3_tight':   dict(family='wide64',  make=('lti', dict(index=20, nx=25, nu=8, Np=3, xbox=1.0)), backends=(None,)),
    'wide_70_10_5':        dict(family='wide128', make=('wide', '80'), backends=(None,)),
    'wide_70_10_5_tight':  dict(family='wide128', make=('lti', dict(index=25, nx=70, nu=10, Np=5, xbox=1.0)), backends=(None,)),
}

# setting -> the cases on which the oracle's counts move within the band: not listed (tests/test_settings_cases.py checks that they do move)
MOVES = {
    'chk1':      ('random_5_3_8', 'quadcopter', 'random_20_8_12', 'cart_pole_nc1', 'group_5_3_40_40'),
    'chk7':      ('quadcopter',),
    'alpha1':    ('quadcopter', 'random_20_8_12'),
    'rho1':      ('quadcopter',),
    'sigma1e-2': ('cart_pole_nc1',),
    'max40':     ('point_mass', 'group_5_3_40_40'),      # (iteration 40 sits on the 10x test / on the exact test of the end-of-run rule)
    'chk0':      ('random_12_4_30_tight', 'wide_25_8_3', 'wide_70_10_5'),      # (rho estimates from residuals at rounding level: the two orders differ)
}

# setting -> the cases on which it cannot be told from the defaults: the same counts, and the same iterate after 40 plain iterations to 1e-4
# relative (a stop schedule the default run never reaches, a regularisation or a fourth Ruiz pass that barely moves an easy problem): not listed
SAME_AS_DEFAULT = {
    'rho30':       ('point_mass', 'quadcopter'),
    'chk10_rho15': ('quadcopter',),
    'sigma1e-2':   ('point_mass', 'random_12_4_30', 'random_12_4_30_hard', 'group_3_2_50_20', 'wide_25_8_3', 'wide_70_10_5'),
    'scaling3':    ('random_12_4_30', 'wide_25_8_3', 'wide_70_10_5'),
    'noadapt':     ('point_mass', 'quadcopter', 'random_12_4_30', 'random_5_3_8_nc', 'group_3_2_50_20', 'group_5_3_40_40', 'wide_25_8_3', 'wide_70_10_5'),
    'max60':       ('quadcopter', 'random_12_4_30', 'group_3_2_50_20', 'group_5_3_40_40', 'wide_25_8_3', 'wide_70_10_5'),
}

# closed loops: STEPS steps of a batch of three copies of the case, x0 scaled by the loop's factors, every copy with the disturbance noise(nx).
# (A factor is replaced like a seed: 1.0 moves wide_25_8_3 under chk1 and chk7, 0.9 moves it under tol1.5 and random_20_8_12 under chk7,
#  0.6 moves cart_pole under alpha1.8.)
STEPS = 6
_F = (1.0, 0.9, 0.6)
_SIX = ('chk1', 'chk7', 'chk10_rho15', 'alpha1.8', 'tol1.5', 'noadapt')
LOOPS = {(c, s): _F for c in ('random_12_4_30', 'group_3_2_50_20', 'wide_25_8_3') for s in _SIX}
LOOPS.update({('wide_25_8_3', 'chk1'): (0.7, 0.6, 1.1), ('wide_25_8_3', 'chk7'): (0.9, 0.7, 0.6), ('wide_25_8_3', 'tol1.5'): (1.0, 0.8, 0.6),
              ('cart_pole', 'alpha1.8'): (1.0, 0.9, 0.5), ('cart_pole', 'tol1.5'): _F,
              ('random_20_8_12', 'chk7'): (1.0, 0.8, 0.6), ('random_20_8_12', 'tol1.5'): _F,      # (one step of tol1.5 runs into max_iter)
              ('random_5_3_8_nc', 'chk7'): _F, ('random_5_3_8_nc', 'alpha1.8'): _F})
LOOP_BACKENDS = {'random_12_4_30': ('bcr8', 'sweeps')}      # (every other loop: the case's first backend)


def settings(name):
    return dict(SETTINGS[name][0]) if name != 'default' else {}


def listed(case):
    """The settings a case is listed for."""
    return [s for s in SETTINGS if case not in MOVES.get(s, ()) and case not in SAME_AS_DEFAULT.get(s, ())]


def pairs():
    """Every listed (case, setting)."""
    return [(c, s) for c in CASES for s in listed(c)]


def device_pairs():
    """Every listed (case, backend, setting)."""
    return [(c, b, s) for c in CASES for b in CASES[c]['backends'] for s in listed(c)]


def loop_backends(case):
    return LOOP_BACKENDS.get(case, CASES[case]['backends'][:1])


def device_loops():
    """Every listed (case, backend, setting) of the closed loops."""
    return [(c, b, s) for (c, s) in LOOPS for b in loop_backends(c)]


def noise(nx):
    """[STEPS, nx] additive plant disturbance of every listed loop."""
    return 0.01 * np.random.default_rng(5).standard_normal((STEPS, nx))


def draw(case):
    """(constructor kwargs of MPCController, attributes to set afterwards) of a case."""
    kind, arg = CASES[case]['make']
    if kind == 'golden':
        from util import load_golden, golden_kwargs
        kw = golden_kwargs(load_golden(arg))
        return dict(kw), dict(kw.attrs)
    if kind == 'group':
        from util import group_kw
        return group_kw(arg), {'SOFT_ON': arg[4]}
    if kind == 'wide':
        from util import wide_kw
        return wide_kw(arg), {}
    from pympc_amd import fixtures
    arg = dict(arg)
    Nc, scale = arg.pop('Nc', None), arg.pop('x0_scale', 1.0)
    kw = dict(fixtures.random_lti(**arg))
    kw['x0'] = scale * kw['x0']
    if Nc is not None:
        kw['Nc'] = Nc
    return kw, {}


def controller(case, setting, oracle, eps=EPS, x0=None, **more):
    """An MPCController of the case with the named setting (not set up): on the CPU oracle, or on the device."""
    from pympc_amd import MPCController
    kw, attrs = draw(case)
    kw.update(eps_abs=eps, eps_rel=eps)
    if x0 is not None:
        kw['x0'] = x0
    K = MPCController(**kw)
    for a, v in attrs.items():
        setattr(K, a, v)
    if oracle:
        from oracle.osqp_oracle import OSQP
        K.prob = OSQP()
    K.solver_settings = dict(settings(setting), **more)
    return K


def infeasible_point_mass(oracle, **st):
    """The infeasible point mass of tests/test_gpu_parity.py (u_{-1} = 5 outside what Delta-u allows), set up and solved under the settings st."""
    from pympc_amd import MPCController, fixtures
    kw = fixtures.point_mass()
    kw['uminus1'] = np.array([5.0])
    K = MPCController(**kw)
    if oracle:
        from oracle.osqp_oracle import OSQP
        K.prob = OSQP()
    K.solver_settings = dict(st)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        K.setup()
    return K


def triple(info):
    return (info.status, int(info.iter), int(info.rho_updates))


_solves, _iterates, _loops = {}, {}, {}


def oracle_solve(case, setting, factor=1.0, ordering='mmd'):
    """The oracle's cold solve of (case, setting) at eps = factor * EPS, made once: (triple, x)."""
    key = (case, setting, factor, ordering)
    if key not in _solves:
        K = controller(case, setting, True, eps=factor * EPS, **({} if ordering == 'mmd' else {'ordering': ordering}))
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            K.setup()
        _solves[key] = (triple(K.res.info), np.array(K.res.x))
    return _solves[key]


def oracle_iterate(case, setting, iters):
    """(x, z, y) of the oracle after `iters` plain iterations from the cold start, unscaled, and its (D, E, c); made once."""
    key = (case, setting, iters)
    if key not in _iterates:
        K = controller(case, setting, True)
        K.setup(solve=False)
        K.prob.iterate(iters)
        x, z, y, _ = K.prob.iterate_state()
        _iterates[key] = (x, z, y, K.prob.scaling())
    return _iterates[key]


def oracle_loop(case, setting, copy, factor=1.0, ordering='mmd'):
    """The oracle's own closed loop of one copy of a listed loop at eps = factor * EPS: the triples of its STEPS + 1 solves; made once."""
    key = (case, setting, copy, factor, ordering)
    if key not in _loops:
        kw, _ = draw(case)
        Ad, Bd = np.asarray(kw['Ad'], dtype=float), np.asarray(kw['Bd'], dtype=float).reshape(np.asarray(kw['Ad']).shape[0], -1)
        x = LOOPS[(case, setting)][copy] * np.asarray(kw['x0'], dtype=float)
        w = noise(Ad.shape[0])
        K = controller(case, setting, True, eps=factor * EPS, x0=x.copy(), **({} if ordering == 'mmd' else {'ordering': ordering}))
        out = []
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            K.setup()
            out.append(triple(K.res.info))
            for k in range(STEPS):
                u = np.array(K.output(), dtype=float).reshape(-1)
                x = Ad @ x + Bd @ u + w[k]
                K.update(x, u)
                out.append(triple(K.res.info))
        _loops[key] = out
    return _loops[key]


def stable(case, setting):
    """Do the oracle's counts of the cold solve stay put across the band and under its other elimination order?  (bool, the triples)"""
    t = [oracle_solve(case, setting, f)[0] for f in BAND] + [oracle_solve(case, setting, ordering=None)[0]]
    return t[0] == t[1] == t[2] == t[3], t


def loop_stable(case, setting):
    t = [[oracle_loop(case, setting, c, f) for c in range(3)] for f in BAND] + [[oracle_loop(case, setting, c, ordering=None) for c in range(3)]]
    return t[0] == t[1] == t[2] == t[3], t
