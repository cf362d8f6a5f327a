"""A linear MPC controller whose model follows the plant: the nonlinear cart pole of examples/example_inverted_pendulum.py under the drop-in
class, relinearised every few steps with MPCController.update_model (mpcqp_update_model: the device re-equilibrates, refactors and keeps its
iterate -- no read-back, no second setup()).

The model is the plant's own equations with the angle-dependent factors frozen at the current state (sin th = sinc(th) th: a quasi-LPV form,
exact at the point of linearisation and without an affine term), sampled by forward Euler like the reference's model.  The pendulum starts 25 degrees from upright; printed: the state cost of the controller that keeps the model linearised at th = 0 and of the one
that follows the plant, along the same run, and the time one relinearisation takes.  (Beyond ~30 degrees the input and input-rate limits
decide the outcome, not the model.)

    python examples/closed_loop_ltv.py [--steps 120] [--every 4] [--theta0 25]
"""
import argparse
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pympc_amd import MPCController, fixtures      # noqa: E402

M, m, b, ft, l, g, Ts = 0.5, 0.2, 0.1, 0.1, 0.3, 9.81, 50e-3     # examples/example_inverted_pendulum.py:10-17


def plant(x, u):
    """the nonlinear pendulum on a cart, one forward-Euler step"""
    F, v, th, om = float(u[0]), x[1], x[2], x[3]
    s, c = np.sin(th), np.cos(th)
    den = M + m * (1.0 - c * c)
    acc = (m * l * s * om ** 2 - m * g * s * c + m * ft * c * om + F - b * v) / den
    alp = ((M + m) * (g * s - ft * om) - m * l * om ** 2 * s * c - (F - b * v) * c) / (l * den)
    return x + Ts * np.array([v, acc, om, alp])


def model_at(x):
    """(Ad, Bd) of the same equations with sin th = sinc(th) th and every other function of (th, om) frozen at x"""
    th, om = x[2], x[3]
    s, c, sinc = np.sin(th), np.cos(th), np.sinc(th / np.pi)
    den = M + m * (1.0 - c * c)
    Ac = np.array([[0, 1, 0, 0],
                   [0, -b / den, -m * g * c * sinc / den, (m * l * om * s + m * ft * c) / den],
                   [0, 0, 0, 1],
                   [0, b * c / (l * den), (M + m) * g * sinc / (l * den), (-(M + m) * ft - m * l * om * s * c) / (l * den)]])
    Bc = np.array([[0.0], [1.0 / den], [0.0], [-c / (l * den)]])
    return np.eye(4) + Ts * Ac, Ts * Bc


def run(kw, steps, every):
    K = MPCController(**kw)
    K.setup()
    x, cost, t_upd, n_upd, bad = np.array(kw['x0'], dtype=float), 0.0, 0.0, 0, 0
    for k in range(steps):
        if every and k % every == 0:
            Ad, Bd = model_at(x)
            t = time.perf_counter()
            K.update_model(Ad=Ad, Bd=Bd, solve=False)          # the solve comes with update(x) below
            t_upd += time.perf_counter() - t; n_upd += 1
        u = K.output()
        x = plant(x, u)
        K.update(x)
        bad += K.res.info.status != 'solved'
        e = x - kw['xref']
        cost += float(e @ kw['Qx'] @ e)
    return x, cost, bad, (t_upd / n_upd * 1e3 if n_upd else 0.0)


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
        for tag, every in (('model linearised at theta = 0', 0), ('relinearised every %d steps' % a.every, a.every)):
            x, cost, bad, ms = run(dict(kw), a.steps, every)
            print('%-32s state cost %9.4f  end state %s  unsolved steps %d%s'
                  % (tag, cost, np.array2string(x, precision=4, suppress_small=True), bad, '  update_model %.3f ms' % ms if every else ''))


if __name__ == '__main__':
    main()
