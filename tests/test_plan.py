"""The plan of a handle (pympc_amd/csrc/mpcqp_plan.h) without a GPU: tests/plan_driver.hip -- a stand-alone host program over the same
header chain as mpcqp.hip -- runs make_plan and the plan's arithmetic on every case of tests/plan_cases.py, and every field equals what the
library's public getters said of that handle on the MI355X (tests/golden/plan_table.json, scripts/record_plan_table.py)."""
import json
import os
import re
import shutil
import subprocess

import pytest

import plan_cases as pc
from util import ROOT, kernel_resources

HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


@pytest.fixture(scope='module')
def driver_out(tmp_path_factory):
    """(one record per case, the two kernel tables): the driver's output on the case list with the table's compute-unit count."""
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip('no hipcc')
    d = tmp_path_factory.mktemp('plan')
    exe, cases = str(d / 'plan_driver'), str(d / 'cases.txt')
    # (host pass only: the device image the kernels' host stubs would register is absent, and nothing here launches one)
    subprocess.run([HIPCC, '--offload-arch=gfx950', '--cuda-host-only', '-std=c++17', '-Wno-unused-value', '-Wl,--unresolved-symbols=ignore-all',
                    os.path.join(ROOT, 'tests', 'plan_driver.hip'), '-o', exe], check=True, timeout=300)
    table = pc.load_table()
    with open(cases, 'w') as f:
        f.write('%d\n' % table['compute_units'] + ''.join(' '.join(map(str, c)) + '\n' for c in pc.CASES))
    r = subprocess.run([exe, cases], check=True, capture_output=True, text=True, timeout=60)
    lines = [json.loads(l) for l in r.stdout.splitlines()]
    assert len(lines) == len(pc.CASES) + 1
    return lines[:-1], lines[-1]


def test_plan_equals_recorded_handles(driver_out):
    rows = pc.load_table()['rows']
    assert pc.load_table()['compute_units'] == pc.NCU
    for got, want in zip(driver_out[0], rows):
        want = {k: v for k, v in want.items() if k != 'case'}
        assert got == want, (rows[driver_out[0].index(got)]['case'], got, want)


def test_every_refusal_is_recorded():
    errors = {r['error'] for r in pc.load_table()['rows'] if r['rc'] != 0}
    assert errors == {'mpcqp_create: bad dimensions', 'mpcqp_create: nx+nu > 128 is not implemented', 'mpcqp_create: unknown mpcqp_settings.backend',
                      'mpcqp_create: backend DENSE is not available for this shape', 'mpcqp_create: backend BCR is not available for this shape',
                      "problem too large for one workgroup's LDS"}


def test_every_table_row_is_some_case(driver_out):
    """Every row of both kernel tables, for LOOP false and true, is the kernel of at least one recorded handle."""
    rows = pc.load_table()['rows']
    named = {k for r in rows if r['rc'] == 0 for k in r['kernel']}
    tables = driver_out[1]
    assert len(tables['kernels_256']) == 50 and len(tables['kernels_512']) == 16
    assert len(set(tables['kernels_256'] + tables['kernels_512'])) == 66
    assert named == set(tables['kernels_256']) | set(tables['kernels_512'])


def test_tables_are_the_instantiations_of_the_build(driver_out):
    """The k_mpc_run and w8::k_mpc_run instantiations the compiler reports for the library are the tables x {false, true}: nothing
    instantiated that no handle can launch, nothing a handle can launch missing."""
    built = set()
    for name in kernel_resources():         # (mangled: _Z9k_mpc_runI... and _ZN2w89k_mpc_runI...)
        m = re.match(r'_Z(N2w8)?9k_mpc_runILi(\d+)ELb([01])ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])EE', name)
        if m:
            w8, nb, ldss, nxt, nut, mode, loop = m.groups()
            tf = {'0': 'false', '1': 'true'}
            built.add('%sk_mpc_run<%s,%s,%s,%s,%s,%s>' % ('w8::' if w8 else '', nb, tf[ldss], nxt, nut, mode, tf[loop]))
    tables = driver_out[1]
    assert sum(k.startswith('w8::') for k in built) == 16
    assert built == set(tables['kernels_256']) | set(tables['kernels_512'])
