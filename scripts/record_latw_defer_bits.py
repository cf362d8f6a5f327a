"""Record the goldens of tests/test_gpu_latw_defer_bits.py with a given build of the library (on the GPU):
    python scripts/record_latw_defer_bits.py <lib.so> [out dir, default tests/golden/latw_defer_bits]
Run it with the build whose bits are to be kept -- the parent commit's, when a change claims to move none."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
from pympc_amd import _lib
_lib.LIB_PATH = os.path.abspath(sys.argv[1])
import numpy as np
import latw_defer_bits_cases as lb

out = sys.argv[2] if len(sys.argv) > 2 else lb.BITS_DIR
os.makedirs(out, exist_ok=True)
for name in lb.CASES:
    arrs, kn = lb.compute(name)
    assert all(np.isfinite(v).all() for v in arrs.values()), name
    p = os.path.join(out, name + '.npz')
    np.savez_compressed(p, kernel=np.array(kn), **arrs)
    if name.startswith('loop_'):
        what = 'carried %d  iterations per step %d .. %d  status %s' % (int(arrs['carried']), arrs['iter'].min(), arrs['iter'].max(), sorted(set(arrs['status'].ravel().tolist())))
    else:
        what = '|x| %.3g' % np.abs(arrs['x%d' % lb.ITERS[-1]]).max()
    print('%-20s %-44s %6d bytes  %s' % (name, kn, os.path.getsize(p), what))
