"""Named solves and closed loops for the bound gradients (include/mpcqp_adjoint_bounds.h): tests/test_bounds_cases.py pins the table on
the CPU oracle, tests/test_gpu_adjoint_bounds.py holds the device to the restatement tests/bounds_ref.py on it.

What the table covers between its entries (asserted by tests/test_bounds_cases.py at eps 1e-9; an entry that stops meeting it is replaced
here, not tolerated there): every listed solve ends 'solved' with no weakly active row even at rollout_cases.WEAK_FACTOR times the device's
weak_tol; each of the six bounds has a non-zero gradient somewhere; the first Delta-u rows are active, lower and upper; a state row is
active with slack columns and one with SOFT_ON = False.

  SINGLE  golden fixtures: cart_pole (upper state rows, slack), random_5_3_8 (state rows on both sides, slack), point_mass_hard (no slack:
          input and Delta-u rows), point_mass_nc (Delta-u rows on both sides, held input) -- and HARD_STATE, point_mass_hard with the velocity
          bound tightened to 0.8 until it binds: no existing fixture has SOFT_ON = False with an active state row.
  ROLLOUT (case, seed) of tests/rollout_cases.py: Delta-u rows on both sides, the first ones included -- their input box of 0.5 sits behind
          the Delta-u box of 0.25 and is never reached, and no state row is ever active.
  LOOPS   closed loops of this table's own: 'xbox_soft', a random plant under a state box of 0.5 (state rows on both sides over its tape,
          with slack columns); 'ubox_tight', one under an input box of 0.2 inside the Delta-u box of 0.25 (input rows on both sides at
          every step, linearly independent active rows); 'hard_state', HARD_STATE stepped: an upper state row active at every step
          without slack columns; 'cart_up', the cart pole's first step (upper state rows alone hold u_0), and 'cart_low', its mirror image
          (lower state rows).
FD_LOOPS: the loops whose restatement is held against central differences of the oracle's loop; their active rows are linearly independent
(where they are not, r_y and with it the split of a gradient between two bounds is not unique: random_lti(7202) under the same boxes
has such a step).  Not among them: 'xbox_soft' -- its x0 lies outside its state box, the rows of stage 0 are held by slack variables under
eps_feas = 1e6 with multipliers of 5e5, and the oracle's 1e-10 relative to those leaves 1e-5 on the trajectory, nothing a step of 1e-6 can
be divided into -- and 'hard_state', where the first Delta-u row pins u_0 at every step, so that the state bound has a zero gradient.
"""
import numpy as np

import util
import rollout_cases as rc

GOLDEN = ('cart_pole', 'random_5_3_8', 'point_mass_hard', 'point_mass_nc')
HARD_STATE = 'point_mass_hard_v08'
SINGLE = GOLDEN + (HARD_STATE,)
ROLLOUT = (('first', 0), ('first', 5), ('held', 3), ('hard', 7), ('nb64', 11), ('nb128', 42))
# name -> the instance, SOFT_ON, steps  (plant = model, no disturbance, constant reference: as tests/rollout_cases.py)
LOOPS = {
    'xbox_soft':  dict(nx=5, nu=3, Np=12, Nc=12, soft=True,  K=4, tv=False),
    'ubox_tight': dict(nx=4, nu=2, Np=10, Nc=10, soft=True,  K=3, tv=False),
    'hard_state': dict(nx=2, nu=1, Np=20, Nc=20, soft=False, K=3, tv=False),
    'cart_up':    dict(nx=4, nu=1, Np=20, Nc=20, soft=True,  K=1, tv=False),
    'cart_low':   dict(nx=4, nu=1, Np=20, Nc=20, soft=True,  K=1, tv=False),
}
FD_LOOPS = ('cart_up', 'cart_low', 'ubox_tight')      # between them every one of the six bounds has a gradient


def single(name):
    """(constructor kwargs, attributes to set afterwards) of one SINGLE entry."""
    from pympc_amd import fixtures
    if name == HARD_STATE:
        kw = dict(fixtures.point_mass())
        kw['xmax'] = np.array([100.0, 0.8])
        return kw, {'SOFT_ON': False}
    kw = util.golden_kwargs(util.load_golden(name))
    return dict(kw), dict(kw.attrs)


def loop(name):
    """(constructor kwargs, attributes to set afterwards) of one LOOPS entry."""
    from pympc_amd import fixtures
    if name == 'xbox_soft':
        return dict(fixtures.random_lti(7201, nx=5, nu=3, Np=12, xbox=0.5, ubox=0.5, dubox=0.25)), {}
    if name == 'ubox_tight':
        return dict(fixtures.random_lti(7200, nx=4, nu=2, Np=10, xbox=4.0, ubox=0.2, dubox=0.25)), {}
    if name in ('cart_up', 'cart_low'):
        kw = dict(fixtures.cart_pole())
        if name == 'cart_low':
            kw.update(x0=-kw['x0'], xref=-kw['xref'], xmin=-kw['xmax'], xmax=-kw['xmin'])
        return kw, {}
    assert name == 'hard_state', name
    return single(HARD_STATE)


def loop_batch_kwargs(name, B=1, **settings):
    """BatchMPCController kwargs of B copies of a loop's instance."""
    kw, attrs = loop(name)
    return util.repeated(kw, B, Nc=None, eps_feas=kw.get('eps_feas', 1e6), SOFT_ON=attrs.get('SOFT_ON', True), **settings)


def row_kinds(nx, nu, Np, Nc):
    """The rows of A by kind, as the builder lays them out (dynamics | state box | input box | Delta-u, tests/adjoint_cases.py):
    dict(state, input, du, du_first) of index arrays."""
    N = Np + 1
    rs, ri, rdu = N * nx, 2 * N * nx, 2 * N * nx + Nc * nu
    m = rdu + (Nc + 1) * nu
    return dict(state=np.arange(rs, ri), input=np.arange(ri, rdu), du=np.arange(rdu, m), du_first=np.arange(rdu, rdu + nu))


def active_by_kind(kw, low, upp):
    """dict kind -> (lower-active rows, upper-active rows) counts of one solve's active set."""
    nx, nu = np.asarray(kw['Bd']).shape
    Np = kw['Np']
    Nc = Np if kw.get('Nc') is None else kw['Nc']
    return {k: (int(np.count_nonzero(low[r])), int(np.count_nonzero(upp[r]))) for k, r in row_kinds(nx, nu, Np, Nc).items()}
