"""include/mpcqp.h is the contract; pympc_amd/_lib.py and the ctypes snippet in INTEGRATION.md are hand-written mirrors of
its structs.  A field added to the header and forgotten in a mirror makes mpcqp_default_settings write past the Python
object (that happened: soft_constraints) -- so the struct layouts are parsed out of the header and compared field by field,
and every function prototype of the header must be bound by _lib.SYMBOLS and vice versa."""
import ctypes as C
import os

from abi import ROOT, header, header_struct, ctypes_struct, header_functions

HEADER = header('mpcqp.h')


def test_ctypes_structs_mirror_the_header():
    from pympc_amd import _lib
    assert ctypes_struct(_lib.Settings) == header_struct(HEADER, 'mpcqp_settings')
    assert ctypes_struct(_lib.Info) == header_struct(HEADER, 'mpcqp_info')
    assert ctypes_struct(_lib.Model) == header_struct(HEADER, 'mpcqp_model')
    assert ctypes_struct(_lib.Loop) == header_struct(HEADER, 'mpcqp_loop')
    # sizes as the C compiler lays them out (natural alignment; no packing pragmas in the header)
    assert C.sizeof(_lib.Settings) == 8 * 8 + 9 * 4 + 4          # 9 int32 + tail padding to 8
    assert C.sizeof(_lib.Info) == 4 * 4 + 4 * 8


def test_symbol_list_is_the_header():
    from pympc_amd import _lib
    assert sorted(_lib.SYMBOLS) == header_functions(HEADER)


def test_integration_doc_snippet_mirrors_the_header():
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    snip = doc[doc.index('class Settings(C.Structure)'):doc.index('s = Settings()')]
    ns = {'C': C}
    exec(snip, ns)
    assert ctypes_struct(ns['Settings']) == header_struct(HEADER, 'mpcqp_settings')
    assert ctypes_struct(ns['Model']) == header_struct(HEADER, 'mpcqp_model')
