"""Record the goldens of tests/test_gpu_latw_bits.py with a given build of the library (on the GPU):
    python scripts/record_latw_bits.py <lib.so> [out dir, default tests/golden/latw_bits]
Run it with the build whose bits are to be kept -- the parent commit's, when a change claims to move none."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
from pympc_amd import _lib
_lib.LIB_PATH = os.path.abspath(sys.argv[1])
import numpy as np
import latw_bits_cases as lb

out = sys.argv[2] if len(sys.argv) > 2 else lb.BITS_DIR
os.makedirs(out, exist_ok=True)
for name in lb.CASES:
    arrs, kn = lb.compute(name)
    assert all(np.isfinite(v).all() for v in arrs.values()), name
    p = os.path.join(out, name + '.npz')
    np.savez_compressed(p, kernel=np.array(kn), **arrs)
    print('%-22s %-40s %6d bytes  |x| %.3g' % (name, kn, os.path.getsize(p), np.abs(arrs['x%d' % lb.ITERS[-1]]).max()))
