"""The top of the latency round (pympc_amd/csrc/mpcqp_latw.h, latw_top_valu) bit for bit against the library that fetched its matrix pairs two column
pairs at a time: with eight waves the top now fetches single pairs, and this test pins that and every later regrouping or earlier request of the top's
LDS reads (one, in front of the top's barrier, was measured and not kept: LAB_NOTES.md; the file keeps the name it was written under).  Closed loops
through mpcqp_mpc_loop on the shapes at which a regrouping can go wrong: the fused schedule, trailing stages absent, an unfused schedule whose last
waves own no group, a top of two column pairs, a refactorization inside the launch, and both ways across the round boundary.  Cases and what each must
show of itself: tests/latw_top_prefetch_cases.py.  The goldens under tests/golden/latw_top_prefetch/ were recorded on an MI355X with
scripts/record_latw_top_prefetch_bits.py and the library as it was BEFORE the grouping changed; a change that is MEANT to move bits re-records them
and says so."""
import numpy as np
import pytest

from latw_top_prefetch_cases import CASES, KEYS, assert_precondition, compute, path

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b)


@pytest.mark.parametrize('name', list(CASES))
def test_top_prefetch_keeps_every_bit(name):
    got, kn = compute(name)
    g = np.load(path(name))
    assert str(g['kernel']) == kn, (str(g['kernel']), kn)
    assert_precondition(name, got, kn)          # (from the handle of THIS run: kernel name, carry counter, mpcqp_get_stats)
    assert_precondition(name, g, kn)
    for k in KEYS:
        assert g[k].dtype == (np.float64 if k in ('x', 'u') else np.int64), (k, g[k].dtype)
        assert same_bits(got[k], g[k]), (name, k, got[k], g[k])
    for k in ('carried', 'checks', 'refactorizations'):
        assert int(got[k]) == int(g[k]), (name, k, int(got[k]), int(g[k]))
