"""The C ABI of msdr_chain_set_decimation, without a GPU: the two symbols with their prototypes, the new flavour bit (an enumerator beside its
four predecessors, so that the header's #define list stays what tests/test_abi.py counts), the maxima, and the Python binding's mirror of them."""
import ctypes as C
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
import msdr  # noqa: E402

HDR = open(os.path.join(ROOT, "include", "msdr.h")).read()
CODE = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)


def test_the_two_symbols_and_their_prototypes():
    lib = msdr.load_library()
    assert re.search(r"\bint\s+msdr_chain_set_decimation\s*\(\s*msdr_chain\s*\*\s*chain\s*,\s*uint32_t\s+D\s*\)\s*;", CODE)
    assert re.search(r"\bint\s+msdr_chain_get_decimation\s*\(\s*msdr_chain\s*\*\s*chain\s*,\s*uint32_t\s*\*\s*D\s*\)\s*;", CODE)
    assert lib.msdr_chain_set_decimation.argtypes == [C.c_void_p, C.c_uint32]
    assert lib.msdr_chain_get_decimation.argtypes == [C.c_void_p, C.c_void_p]
    assert lib.msdr_chain_set_decimation.restype is C.c_int and lib.msdr_chain_get_decimation.restype is C.c_int
    assert callable(msdr.Chain.set_decimation) and callable(msdr.Chain.decimation)


def test_a_null_chain_is_an_argument_error_without_a_device():
    lib = msdr.load_library()
    d = C.c_uint32(7)
    assert lib.msdr_chain_set_decimation(None, C.c_uint32(4)) == msdr.STATUS_ARGUMENT_ERROR
    assert lib.msdr_last_error()
    assert lib.msdr_chain_get_decimation(None, C.byref(d)) == msdr.STATUS_ARGUMENT_ERROR and d.value == 7


def test_the_flavour_bit_is_an_enumerator_and_the_binding_mirrors_the_header():
    m = re.search(r"enum\s*\{\s*MSDR_FLAVOUR_DECIMATED\s*=\s*(0x[0-9a-fA-F]+)u\s*\}\s*;", CODE)
    assert m and int(m.group(1), 16) == 0x100000 == msdr.FLAVOUR_DECIMATED
    assert not re.search(r"#define\s+MSDR_FLAVOUR_DECIMATED", HDR)
    # no other flavour bit has the value
    others = {n: int(v, 0) for n, v in re.findall(r"MSDR_(FLAVOUR_[A-Z_]+)\s*=?\s+(0x[0-9a-fA-F]+)u", CODE) if n != "FLAVOUR_DECIMATED"}
    assert len(others) >= 16 and all(v != 0x100000 for v in others.values()), others
    m = re.search(r"enum \{ MSDR_MAX_DECIMATION_Q15 = (\d+), MSDR_MAX_DECIMATION_F32 = (\d+) \};", CODE)
    assert m and (int(m.group(1)), int(m.group(2))) == (msdr.MAX_DECIMATION_Q15, msdr.MAX_DECIMATION_F32)
