"""The shipped library's plans against tests/golden/plan_table.json: for every case of tests/plan_cases.py a handle is created (never set up,
never solved) and the public getters must say what they said when the table was recorded.  tests/test_plan.py ties the device-free
make_plan to the same table; this ties the library."""
import pytest

import plan_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    from pympc_amd import _lib
    return _lib.load(), _lib.Settings


def test_device_has_the_tables_compute_units(lib):
    L, Settings = lib
    got = pc.handle_record(L, Settings, pc.CASES[0])
    assert got['occupancy'][1] == pc.load_table()['compute_units'] == pc.NCU


def test_getters_equal_the_table(lib):
    L, Settings = lib
    for want in pc.load_table()['rows']:
        assert pc.handle_record(L, Settings, tuple(want['case'])) == want
