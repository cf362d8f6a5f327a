"""Record the golden of tests/test_gpu_rollout_tv.py::test_the_unscheduled_sweep_has_the_bits_it_had with a given build of the library (on
the GPU):
    python scripts/record_rollout_const_bits.py <lib.so> [out file, default tests/golden/rollout_const_bits.npz]
Run it with the build whose bits are to be kept -- the parent commit's, when a change to the sweep's body (a new template parameter of
rollout_adjoint_body, pympc_amd/csrc/mpcqp_rollout.h) claims to move none of k_rollout_adjoint<NB>'s.

``outputs()`` is what the test compares: rollout() of case 'first' of tests/rollout_cases.py with a disturbance and its own plant, then
rollout_adjoint for every gradient it has on a tape without a schedule or an estimator, the bounds included, per instance and summed over
the batch."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
import numpy as np

WANT = ('lam', 'uminus1', 'uref', 'xref', 'Ap', 'Bp', 'Ad', 'Bd', 'Qx', 'QxN', 'Qu', 'QDu', 'eps_feas', 'xmin', 'xmax', 'umin', 'umax', 'Dumin', 'Dumax')
SUMMED = WANT[6:]
OUT = os.path.join(ROOT, 'tests', 'golden', 'rollout_const_bits.npz')


def outputs():
    """name -> array: the forward trajectories, the sweep's gradients, its per-step counts, and the batch sums."""
    import rollout_cases as rc
    import rollout_dev
    name = rc.FIRST
    K = rc.CASES[name]['K']
    io = rollout_dev.inputs(name, True, True)
    C = rollout_dev.ctrl(name)
    tr = C.rollout(K, w=io['w'], Ap=io['Ap'], Bp=io['Bp'])
    rng = np.random.default_rng(41)
    gx, gu = rng.standard_normal((K + 1, C.B, C.nx)), rng.standard_normal((K, C.B, C.nu))
    res = dict(x=tr['x'], u=tr['u'], iter=tr['iter'])
    got = C.rollout_adjoint(g_x=gx, g_u=gu, want=WANT)
    res.update({k: got[k] for k in WANT + ('n_weak', 'status', 'n_factor')})
    tot = C.rollout_adjoint(g_x=gx, g_u=gu, want=SUMMED, batch_sum=True)
    res.update({'sum_' + k: tot[k] for k in SUMMED})
    plain = rollout_dev.ctrl(name)                         # the plant is the model, no disturbance: the sweep reads Ad, Bd out of LDS
    plain.rollout(K)
    got = plain.rollout_adjoint(g_x=gx, g_u=gu, want=WANT)
    res.update({'plain_' + k: got[k] for k in WANT + ('n_factor',)})
    return {k: np.ascontiguousarray(v) for k, v in res.items()}


if __name__ == '__main__':
    from pympc_amd import _lib
    _lib.LIB_PATH = os.path.abspath(sys.argv[1])
    out = sys.argv[2] if len(sys.argv) > 2 else OUT
    arrs = outputs()
    assert all(np.isfinite(v).all() for v in arrs.values())
    os.makedirs(os.path.dirname(out), exist_ok=True)
    np.savez_compressed(out, **arrs)
    print('%s: %d arrays, %d bytes, n_factor %s, |lam| %.3g' % (out, len(arrs), os.path.getsize(out), arrs['n_factor'].tolist(), np.abs(arrs['lam']).max()))
