"""Restatement of the bound gradients (include/mpcqp_adjoint_bounds.h) for the tests: numpy only, sharing nothing with the HIP kernel
(pympc_amd/csrc/mpcqp_adjoint_bounds.h).

dL/db_r = r_y[r] on the active rows (tests/adjoint_ref.py: d_l on a lower-active or equality row, d_u on an upper-active one), and l, u are
affine in xmin, xmax, umin, umax, Dumin, Dumax.  Which row carries which bound is not written down here: the Jacobians of l, u are read
off the host builder (pympc_amd.qp_build through MPCController._compute_QP_matrices_) by moving one bound entry at a time by one unit, as
adjoint_ref.parameter_maps does for the step data.  1.0 is a power of two and the map is affine, so the differences are exact; an infinite
entry does not move and gives a zero column.

A sweep's gradients are the recursion of tests/rollout_ref.py (tests/rollout_est_ref.py) with the step's gradients added per solved entry:
the bounds are constant over the tape.  Those modules return the sums, not the r_y of each entry, so the sweep here runs them with a recorder
around adjoint_ref.adjoint that keeps the d_l, d_u of every entry they solve -- the same solves, nothing recomputed.
"""
import contextlib

import numpy as np

import adjoint_ref
import adjoint_model_ref
import rollout_ref
import rollout_est_ref

NAMES = ('xmin', 'xmax', 'umin', 'umax', 'Dumin', 'Dumax')


def bound_maps(kw, attrs=None):
    """Jacobians of (l, u) with respect to the six bounds: dict name -> (Jl [m, p], Ju [m, p]), p = nx or nu.  kw: constructor kwargs of the
    controller (a bound it does not give is infinite: zero columns)."""
    kw = adjoint_model_ref.full_kwargs(kw)
    nx, nu = kw['Bd'].shape
    _, l0, u0 = _vectors(kw, attrs)
    maps = {}
    for name in NAMES:
        p = nx if name in ('xmin', 'xmax') else nu
        Jl, Ju = np.zeros((l0.size, p)), np.zeros((u0.size, p))
        if kw.get(name) is not None:
            base = np.array(kw[name], dtype=float)
            for j in range(p):
                v = base.copy(); v[j] += 1.0
                _, l1, u1 = _vectors(dict(kw, **{name: v}), attrs)
                Jl[:, j], Ju[:, j] = adjoint_model_ref._fin_diff(l1, l0), adjoint_model_ref._fin_diff(u1, u0)
        maps[name] = (Jl, Ju)
    return maps


def _vectors(kw, attrs):
    (_, q, _, l, u), _ = adjoint_model_ref.build(kw, attrs)
    return q, l, u


def chain(maps, d_l, d_u):
    """dL/d(bound) = Jl' d_l + Ju' d_u.  (A row given equal bounds has its derivative in d_l and 0 in d_u: the lower name gets it.)"""
    return {name: Jl.T @ d_l + Ju.T @ d_u for name, (Jl, Ju) in maps.items()}


def step(maps, r):
    """The six gradients of one solve from what adjoint_ref.adjoint returned for one seed."""
    return chain(maps, r['d_l'], r['d_u'])


@contextlib.contextmanager
def _recorded():
    calls, orig = [], adjoint_ref.adjoint

    def rec(*a, **k):
        r = orig(*a, **k)
        calls.append((np.array(r['d_l'], dtype=float), np.array(r['d_u'], dtype=float)))
        return r
    adjoint_ref.adjoint = rec
    try:
        yield calls
    finally:
        adjoint_ref.adjoint = orig


def _summed(res, calls, bmaps):
    assert len(calls) == res['n_solved'], (len(calls), res['n_solved'])
    tot = {n: np.zeros(J[0].shape[1]) for n, J in bmaps.items()}
    for d_l, d_u in calls:                                   # (in the sweep's order: K-1 .. 0 over the solved entries)
        for n, v in chain(bmaps, d_l, d_u).items():
            tot[n] = tot[n] + v
    res.update(tot)
    return res


def sweep(kw, attrs, tape, D, E, c, *args, bmaps=None, **kwargs):
    """rollout_ref.sweep with the six bound gradients, summed over the solved entries, added to its dict."""
    bmaps = bound_maps(rollout_ref.entry_kwargs(kw, tape[0]), attrs) if bmaps is None else bmaps
    with _recorded() as calls:
        res = rollout_ref.sweep(kw, attrs, tape, D, E, c, *args, **kwargs)
    return _summed(res, calls, bmaps)


def sweep_est(kw, attrs, tape, D, E, c, C, L, *args, bmaps=None, **kwargs):
    """rollout_est_ref.sweep likewise."""
    bmaps = bound_maps(rollout_ref.entry_kwargs(kw, tape[0]), attrs) if bmaps is None else bmaps
    with _recorded() as calls:
        res = rollout_est_ref.sweep(kw, attrs, tape, D, E, c, C, L, *args, **kwargs)
    return _summed(res, calls, bmaps)
