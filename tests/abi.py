"""What the ABI tests share (tests/test_abi_layout.py and the test_*_abi.py next to it): the parsers that read struct layouts and function
prototypes out of include/*.h, the ctypes side of the same comparison, the pinned hashes of the headers an extension must leave alone,
and the ``twin`` fixture that binds pympc_amd to the CPU twin for one test.  A test module that uses the fixture imports it by name."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the headers the adjoint extension sits beside, as they were before it (sha256 of the files) ...
OLDER_HEADERS = {
    'mpcqp.h': '9b65550ae4f89a6a8ef2d36876ae97a0bc26d31d994514d8c3a1c1ab8e0832a8',
    'mpcqp_polish.h': '8fdf6b5c286dbd74132ab41a8a18616ed4bb5d73233d1fd209293d46fbc682ad',
    'mpcqp_model.h': '2803bb5b65ee660e7da727e459a53997cd7f6d3d0f702b18a04a1bc6b7bb2692',
}
# ... and the two that came after, as the extensions after them found them
ADJOINT_HEADER_SHA256 = 'e0292e51830ab2f92d7424665564e3b43597b7adc9f9423074a940eb6387a585'
ADJOINT_MODEL_HEADER_SHA256 = 'f76953e39fa025bfa214a6583c869c633d8a432f86e2631fac754d6156cbdc41'


def header(name):
    """The text of include/<name>."""
    return open(os.path.join(ROOT, 'include', name)).read()


def strip_comments(text):
    return re.sub(r'/\*.*?\*/', '', text, flags=re.S)


def header_struct(text, name):
    """[(field, kind)] of `typedef struct { ... } name;` in a header's text, kind in {'double', 'int32', 'ptr'}."""
    body = re.search(r'typedef struct \{([^{}]*)\}\s*%s\s*;' % name, strip_comments(text)).group(1)
    fields = []
    for decl in body.split(';'):
        decl = ' '.join(decl.split())
        if not decl:
            continue
        m = re.match(r'(const )?(double|int32_t)\s*(.*)', decl)
        assert m, decl
        base = m.group(2)
        for item in m.group(3).split(','):
            item = item.strip()
            ptr = item.startswith('*')
            fields.append((item.lstrip('* ').strip(), 'ptr' if ptr else ('double' if base == 'double' else 'int32')))
    return fields


def ctypes_struct(cls):
    """The same list of a ctypes.Structure."""
    kind = lambda t: 'double' if t is C.c_double else ('int32' if t in (C.c_int32, C.c_int) else 'ptr')
    return [(n, kind(t)) for n, t in cls._fields_]


def header_functions(text):
    """Sorted names of the mpcqp_* functions a header's text declares."""
    text = re.sub(r'typedef struct \{.*?\}\s*\w+\s*;', '', strip_comments(text), flags=re.S)
    return sorted(set(re.findall(r'\b(mpcqp_\w+)\s*\(', text)))


def lib_loaded():
    """(pympc_amd._lib, the loaded HIP library), built first if it is not there."""
    import __graft_entry__ as g
    from pympc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib, _lib.load()


@pytest.fixture
def twin():
    """pympc_amd bound to the CPU twin for one test (the product loader itself reads no switch: the test swaps the path)."""
    from pympc_amd import _lib
    subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'oracle'), 'libmpcqp_cpu.so'])
    old = (_lib.LIB_PATH, _lib._lib)
    _lib.LIB_PATH, _lib._lib = os.path.join(ROOT, 'oracle', 'libmpcqp_cpu.so'), None
    try:
        yield _lib.load()
    finally:
        _lib.LIB_PATH, _lib._lib = old
