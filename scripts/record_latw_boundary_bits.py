"""Record the goldens of tests/test_gpu_latw_boundary_bits.py with a given build of the library (on the GPU):
    python scripts/record_latw_boundary_bits.py <lib.so> [out dir, default tests/golden/latw_boundary]
Run it with the build whose bits are to be kept -- the parent commit's, when a change claims to move none.  Refuses a run in which some exit of the
round boundary does not occur (tests/latw_boundary_cases.py: assert_classes)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
from pympc_amd import _lib
_lib.LIB_PATH = os.path.abspath(sys.argv[1])
import numpy as np
import latw_boundary_cases as lb

out = sys.argv[2] if len(sys.argv) > 2 else lb.BOUNDARY_DIR
os.makedirs(out, exist_ok=True)
runs = {}
for name in lb.CASES:
    runs[name], kn = lb.compute(name)
    assert kn.startswith('w8::k_mpc_run<16,') and kn.endswith(lb.kernel_suffix(name)), kn
    p = os.path.join(out, name + '.npz')
    np.savez_compressed(p, kernel=np.array(kn), **runs[name])
    print('%-14s %-44s %6d bytes\n    status %s\n    iter   %s' % (name, kn, os.path.getsize(p), runs[name]['status'].T.tolist(), runs[name]['iter'].T.tolist()), flush=True)
    print('    %s' % lb.classes(name, runs[name]), flush=True)
lb.assert_classes(runs)
print('every exit occurs')
