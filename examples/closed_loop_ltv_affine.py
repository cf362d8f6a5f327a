"""A linear MPC controller relinearised by the plant's TRUE Jacobians: the nonlinear cart pole of examples/closed_loop_ltv.py under the drop-in
class, with the model  x+ = A x + B u + c  taken at the current (x, u) every few steps -- A = df/dx, B = df/du by central differences of the
plant's own step, c = f(x, u) - A x - B u, the offset a linearisation away from an equilibrium always has -- and handed to the controller as
update_model(Ad=A, Bd=B) and update(x, d=c) (mpcqp_set_affine, include_ext4/mpcqp_affine.h: the offset is step data, it costs no factorization).

examples/closed_loop_ltv.py gets round the offset with a quasi-LPV rewriting of this plant (sin th = sinc(th) th), a trick few plants allow.
Printed: the state cost of three controllers along the same run -- the model linearised at th = 0 and never changed, the quasi-LPV model,
and the true Jacobians with their offset.  On this plant, from 25 degrees, relinearised every 4 steps: 1.72, 1.62 and 3.27 with no unsolved
step -- a tangent model held over a horizon of 20 steps extrapolates worse from a point far from the equilibrium than the rewriting made for this
plant, which keeps the origin an equilibrium of every model; the tangent model with its offset is the one that exists for any plant.

    python examples/closed_loop_ltv_affine.py [--steps 120] [--every 4] [--theta0 25]
"""
import argparse
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pympc_amd import MPCController, fixtures      # noqa: E402
from closed_loop_ltv import plant, model_at        # noqa: E402


def jacobians_at(x, u, h=1e-6):
    """(A, B, c) of the plant's step f at (x, u): central differences, and the offset c = f(x, u) - A x - B u"""
    nx, nu = x.size, u.size
    A, B = np.zeros((nx, nx)), np.zeros((nx, nu))
    for j in range(nx):
        e = np.zeros(nx); e[j] = h
        A[:, j] = (plant(x + e, u) - plant(x - e, u)) / (2 * h)
    for j in range(nu):
        e = np.zeros(nu); e[j] = h
        B[:, j] = (plant(x, u + e) - plant(x, u - e)) / (2 * h)
    return A, B, plant(x, u) - A @ x - B @ u


def run(kw, steps, every, mode):
    K = MPCController(**kw)
    K.setup()
    x, cost, bad, c = np.array(kw['x0'], dtype=float), 0.0, 0, None
    for k in range(steps):
        u = np.atleast_1d(np.array(K.output(), dtype=float))
        if mode != 'fixed' and k % every == 0:
            if mode == 'lpv':
                Ad, Bd = model_at(x)
            else:
                Ad, Bd, c = jacobians_at(x, u)
            K.update_model(Ad=Ad, Bd=Bd, solve=False)          # the solve comes with update(x) below
        x = plant(x, u)
        K.update(x, d=c)                                       # (d=None: no term, or the one in force)
        bad += K.res.info.status != 'solved'
        e = x - kw['xref']
        cost += float(e @ kw['Qx'] @ e)
    return x, cost, bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=120)
    ap.add_argument('--every', type=int, default=4, help='relinearise every this many steps')
    ap.add_argument('--theta0', type=float, default=25.0, help='initial angle in degrees')
    a = ap.parse_args()
    kw = fixtures.cart_pole()
    kw['x0'] = np.array([0.0, 0.0, np.deg2rad(a.theta0), 0.0])
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for tag, mode in (('model linearised at theta = 0', 'fixed'), ('quasi-LPV, every %d steps' % a.every, 'lpv'),
                          ('true Jacobians + offset, every %d steps' % a.every, 'affine')):
            x, cost, bad = run(dict(kw), a.steps, a.every, mode)
            print('%-40s state cost %9.4f  end state %s  unsolved steps %d'
                  % (tag, cost, np.array2string(x, precision=4, suppress_small=True), bad))


if __name__ == '__main__':
    main()
