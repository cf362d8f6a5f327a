"""Record the goldens of tests/test_gpu_latw_top_prefetch_bits.py with a given build of the library (on the GPU):
    python scripts/record_latw_top_prefetch_bits.py <lib.so> [out dir, default tests/golden/latw_top_prefetch]
Run it with the build whose bits are to be kept -- the parent commit's, when a change claims to move none.  Refuses a run that does not take
the path its case is about (tests/latw_top_prefetch_cases.py: assert_precondition)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
from pympc_amd import _lib
_lib.LIB_PATH = os.path.abspath(sys.argv[1])
import numpy as np
import latw_top_prefetch_cases as lp

out = sys.argv[2] if len(sys.argv) > 2 else lp.PREFETCH_DIR
os.makedirs(out, exist_ok=True)
for name in lp.CASES:
    arrs, kn = lp.compute(name)
    p = os.path.join(out, name + '.npz')
    np.savez_compressed(p, kernel=np.array(kn), **arrs)
    print('%-18s %-44s %6d bytes  carried %d  checks %d  refactorizations %d\n    status %s\n    iter   %s'
          % (name, kn, os.path.getsize(p), int(arrs['carried']), int(arrs['checks']), int(arrs['refactorizations']),
             arrs['status'].T.tolist(), arrs['iter'].T.tolist()), flush=True)
    lp.assert_precondition(name, arrs, kn)
print('every case takes its path')
