"""The latency round's own termination test (latw_check, pympc_amd/csrc/mpcqp_latw_check.h) in two stages -- the residuals, their scales and the
objective always; the cheap halves of the two infeasibility certificates only where the solve has not converged -- bit for bit against the test that
reduced all twelve values at once.  Splitting the reduction moves no summand and no order of any sum, and a maximum is the same in any grouping; what
it can break is a verdict (a value read from the wrong slot of the reduction, a certificate judged on stale values) or the LDS hand-over between the
two reductions.  The cases (tests/latw_check_stages_cases.py) take every exit of the test: solved at the first check and at the second, a carried
step, one handed back, the primal certificate's cheap half under a hard state box, a non-finite residual.  The goldens under tests/golden/latw_check_stages/ were
recorded on an MI355X with scripts/record_latw_check_stages.py and the library as it was BEFORE the test was split; a change that is MEANT to move
bits re-records them and says so."""
import numpy as np
import pytest

from latw_check_stages_cases import CASES, FLOAT_KEYS, INT_KEYS, assert_classes, compute, path

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b)


def test_recorded_runs_take_every_exit():
    assert_classes({name: np.load(path(name)) for name in CASES})


@pytest.mark.parametrize('name', list(CASES))
def test_closed_loop_keeps_every_bit(name):
    nx, nu, Np, hard, mode = CASES[name]
    got, kn = compute(name)
    g = np.load(path(name))
    assert kn.startswith('w8::k_mpc_run<16,') and kn.endswith(',0,0,%d,true>' % mode), kn
    assert str(g['kernel']) == kn, (str(g['kernel']), kn)
    for k in FLOAT_KEYS + INT_KEYS:
        assert g[k].dtype == (np.float64 if k in FLOAT_KEYS else np.int64), (k, g[k].dtype)
        assert same_bits(got[k], g[k]), (name, k, got[k], g[k])
