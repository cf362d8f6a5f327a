"""Record tests/golden/plan_table.json with a given build of the library (on the GPU):
    python scripts/record_plan_table.py <lib.so> [out file, default tests/golden/plan_table.json]
For every case of tests/plan_cases.py a handle is created -- never set up, never solved -- and what the public getters say of it is kept.
Run it with the build whose plans are to be kept -- the parent commit's, when a change claims to move none."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests'))
from pympc_amd import _lib
_lib.LIB_PATH = os.path.abspath(sys.argv[1])
import plan_cases as pc

L = _lib.load()
out = sys.argv[2] if len(sys.argv) > 2 else pc.TABLE
rows = [pc.handle_record(L, _lib.Settings, c) for c in pc.CASES]
ncu = {r['occupancy'][1] for r in rows if r['rc'] == 0}
assert ncu == {pc.NCU}, ncu
with open(out, 'w') as f:
    f.write('{"compute_units": %d, "rows": [\n%s\n]}\n' % (pc.NCU, ',\n'.join(json.dumps(r) for r in rows)))
print('%d cases (%d refused) -> %s' % (len(rows), sum(r['rc'] != 0 for r in rows), out))
