"""Record the goldens of tests/test_gpu_latw_check_stages.py with a given build of the library (on the GPU):
    python scripts/record_latw_check_stages.py <lib.so> [out dir, default tests/golden/latw_check_stages]
Run it with the build whose bits are to be kept -- the parent commit's, when a change claims to move none.  Refuses a run in which some exit of the
round's termination test does not occur (tests/latw_check_stages_cases.py: assert_classes)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
from pympc_amd import _lib
_lib.LIB_PATH = os.path.abspath(sys.argv[1])
import numpy as np
import latw_check_stages_cases as lc

out = sys.argv[2] if len(sys.argv) > 2 else lc.STAGES_DIR
os.makedirs(out, exist_ok=True)
runs = {}
for name in lc.CASES:
    runs[name], kn = lc.compute(name)
    p = os.path.join(out, name + '.npz')
    np.savez_compressed(p, kernel=np.array(kn), **runs[name])
    print('%-14s %-44s %6d bytes  %s\n    status %s\n    iter   %s' % (name, kn, os.path.getsize(p), lc.classes(name, runs[name]),
          runs[name]['status'].T.tolist(), runs[name]['iter'].T.tolist()), flush=True)
lc.assert_classes(runs)
print('every exit occurs')
