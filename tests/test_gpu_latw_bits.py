"""The latency round (pympc_amd/csrc/mpcqp_latw.h) bit for bit against recorded iterates: changes to HOW it reads its LDS vectors, schedules its
MFMAs or places its waits touch no arithmetic, so x, z and y after 1, 8 and 33 plain ADMM iterations (three mpcqp_iterate calls on one handle) must
keep every bit -- on one smallest shape per schedule: the specialised (12,4,30) instantiation and a generic shape on 31 stages (fused schedule,
five barriers), 21 and 11 stages (seven barriers) on 512-thread workgroups, and (12,4,30) on the 256-thread build.  The goldens under
tests/golden/latw_bits/ were recorded on an MI355X with scripts/record_latw_bits.py and the library as it was BEFORE the round's input vectors became single
8-byte LDS reads (round 8, LAB_NOTES.md); a change that is MEANT to move bits re-records them and says so."""
import numpy as np
import pytest

from latw_bits_cases import CASES, ITERS, BATCH, compute, path

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', list(CASES))
def test_iterates_keep_every_bit(name):
    nx, nu, Np, backend, mode = CASES[name]
    got, kn = compute(name)
    spec = (nx, nu) if name.startswith('spec_') else (0, 0)
    assert kn.startswith('w8::k_mpc_run<16,' if backend == 'bcr8' else 'k_mpc_run<16,') and kn.endswith(',%d,%d,%d,false>' % (spec[0], spec[1], mode)), kn
    g = np.load(path(name))
    assert str(g['kernel']) == kn, (str(g['kernel']), kn)
    for k in ITERS:
        for tag in 'xzy':
            a, b = got['%s%d' % (tag, k)], g['%s%d' % (tag, k)]
            assert a.shape == b.shape and a.shape[0] == BATCH and a.dtype == b.dtype == np.float64, (tag, k, a.shape, b.shape)
            # (the first iteration leaves x = 0: these problems have q = 0, the initial state enters through the bounds and reaches x with the second)
            assert np.isfinite(b).all() and (k == ITERS[0] or np.abs(b).max() > 0), (tag, k)
            assert np.array_equal(a.view(np.int64), b.view(np.int64)), (name, tag, k, int((a.view(np.int64) != b.view(np.int64)).sum()), float(np.abs(a - b).max()))
