"""The round boundary of the latency round (latw_check and latw_carry, pympc_amd/csrc/mpcqp_latw_check.h) bit for bit under dense weights: P x as
one branch-free dot product per lane, barriers that wait for LDS only, the check's own two-barrier reduction and the hand-over move no summand, no
order of a sum and no stored value.  What they can break is an operand taken from the wrong column, stage or neighbour (off-diagonal Qx, QxN != Qx,
dense Qu and QDu make every such slip visible where the benchmark's diagonal weights multiply it by zero), a term added where none is due, a value
read across a barrier that no longer orders it, or a verdict.  Cases and exits: tests/latw_boundary_cases.py.  The goldens under
tests/golden/latw_boundary/ were recorded on an MI355X with scripts/record_latw_boundary_bits.py and the library as it was BEFORE the boundary was
rewritten; a change that is MEANT to move bits re-records them and says so."""
import numpy as np
import pytest

from latw_boundary_cases import CASES, FLOAT_KEYS, INT_KEYS, compute, kernel_suffix, path

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b)


@pytest.mark.parametrize('name', list(CASES))
def test_boundary_keeps_every_bit(name):
    got, kn = compute(name)
    g = np.load(path(name))
    assert kn.startswith('w8::k_mpc_run<16,') and kn.endswith(kernel_suffix(name)), kn
    assert str(g['kernel']) == kn, (str(g['kernel']), kn)
    for k in FLOAT_KEYS + INT_KEYS:
        assert g[k].dtype == (np.float64 if k in FLOAT_KEYS else np.int64), (k, g[k].dtype)
        assert same_bits(got[k], g[k]), (name, k, got[k], g[k])
