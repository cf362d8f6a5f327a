"""The fused schedule of the latency round (pympc_amd/csrc/mpcqp_latw.h) with a leaf product D^-1 b deferred -- level 1's runs at the head of the top;
level 0's were tried in level 1 forward and stayed where they were -- bit for bit against the schedule that ran it where its input was made.  Moving a
product moves no summand and no order of any sum; what it can break is an LDS hazard: tb at 4r+1 (for level 0's leaves: at 4w, 4w+2) is read, and cb
written, a phase later.  tests/test_gpu_latw_bits.py
pins the full 31-stage shapes over plain iterations; here are the shapes and paths it does not reach (tests/latw_defer_bits_cases.py): trailing
stages absent, mostly dead owner lanes, and closed loops whose steps are carried and whose rounds end inside the kernel (the termination test and the
carry reuse the round's vectors).  The goldens under tests/golden/latw_defer_bits/ were recorded on an MI355X with scripts/record_latw_defer_bits.py
and the library as it was BEFORE any product moved; a change that is MEANT to move bits re-records them and says so."""
import numpy as np
import pytest

from latw_defer_bits_cases import CASES, ITERS, BATCH, STEPS, compute, path

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b)


def check_kernel(name, kn, g, loop):
    nx, nu, Np, backend, mode = CASES[name]
    spec = (nx, nu) if (nx, nu, Np) == (12, 4, 30) else (0, 0)
    assert kn.startswith('w8::k_mpc_run<16,') and kn.endswith(',%d,%d,%d,%s>' % (spec[0], spec[1], mode, 'true' if loop else 'false')), kn
    assert str(g['kernel']) == kn, (str(g['kernel']), kn)


@pytest.mark.parametrize('name', [n for n in CASES if n.startswith('iter_')])
def test_iterates_keep_every_bit(name):
    got, kn = compute(name)
    g = np.load(path(name))
    check_kernel(name, kn, g, loop=False)
    for k in ITERS:
        for tag in 'xzy':
            a, b = got['%s%d' % (tag, k)], g['%s%d' % (tag, k)]
            assert a.shape[0] == BATCH and b.dtype == np.float64, (tag, k, a.shape, b.dtype)
            # (the first iteration leaves x = 0: these problems have q = 0, the initial state enters through the bounds and reaches x with the second)
            assert np.isfinite(b).all() and (k == ITERS[0] or np.abs(b).max() > 0), (tag, k)
            assert same_bits(a, b), (name, tag, k, float(np.abs(a - b).max()))


@pytest.mark.parametrize('name', [n for n in CASES if n.startswith('loop_')])
def test_closed_loop_keeps_every_bit(name):
    got, kn = compute(name)
    g = np.load(path(name))
    check_kernel(name, kn, g, loop=True)
    # the recorded run is the one this test is about: steps carried inside the round, and more than one round per step
    assert g['x'].shape[:2] == (STEPS + 1, BATCH) and int(g['carried']) > 0 and (g['status'] == 1).all() and g['iter'].min() > 0, (g['x'].shape, int(g['carried']))
    assert int(got['carried']) == int(g['carried']), (int(got['carried']), int(g['carried']))
    for k in ('x', 'u', 'status', 'iter'):
        assert np.isfinite(g[k]).all() and same_bits(got[k], g[k]), (name, k)
