"""The C ABI of msdr_chain_set_prefilter, without a GPU: the three symbols with their prototypes, the new flavour bit (an enumerator beside its
predecessors, so that the header's #define list stays what tests/test_abi.py counts), the Python binding and the host node's mirror of them,
and every refusal that needs no device."""
import ctypes as C
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
import msdr  # noqa: E402

HDR = open(os.path.join(ROOT, "include", "msdr.h")).read()
CODE = re.sub(r"/\*.*?\*/", "", HDR, flags=re.S)
NODES = open(os.path.join(ROOT, "minimal-sdr_amd", "host", "msdr_nodes.h")).read()


def test_the_three_symbols_and_their_prototypes():
    lib = msdr.load_library()
    assert re.search(r"\bint\s+msdr_chain_set_prefilter\s*\(\s*msdr_chain\s*\*\s*chain\s*,\s*uint32_t\s+D1\s*,\s*uint32_t\s+num_taps\s*,\s*const\s+int16_t\s*\*\s*taps\s*\)\s*;", CODE)
    assert re.search(r"\bint\s+msdr_chain_set_prefilter_f32\s*\(\s*msdr_chain\s*\*\s*chain\s*,\s*uint32_t\s+D1\s*,\s*uint32_t\s+num_taps\s*,\s*const\s+float\s*\*\s*taps\s*\)\s*;", CODE)
    assert re.search(r"\bint\s+msdr_chain_get_prefilter\s*\(\s*msdr_chain\s*\*\s*chain\s*,\s*uint32_t\s*\*\s*D1\s*,\s*uint32_t\s*\*\s*num_taps\s*\)\s*;", CODE)
    for name in ("msdr_chain_set_prefilter", "msdr_chain_set_prefilter_f32"):
        f = getattr(lib, name)
        assert f.argtypes == [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p] and f.restype is C.c_int, name
    assert lib.msdr_chain_get_prefilter.argtypes == [C.c_void_p, C.c_void_p, C.c_void_p] and lib.msdr_chain_get_prefilter.restype is C.c_int
    assert callable(msdr.Chain.set_prefilter) and callable(msdr.Chain.prefilter)


def test_a_null_chain_is_an_argument_error_without_a_device():
    lib = msdr.load_library()
    taps16 = (C.c_int16 * 8)(*([0] * 7 + [32767]))
    tapsf = (C.c_float * 8)(*([0.0] * 7 + [1.0]))
    d, n = C.c_uint32(7), C.c_uint32(9)
    assert lib.msdr_chain_set_prefilter(None, C.c_uint32(8), C.c_uint32(8), taps16) == msdr.STATUS_ARGUMENT_ERROR
    assert lib.msdr_last_error()
    assert lib.msdr_chain_set_prefilter_f32(None, C.c_uint32(8), C.c_uint32(8), tapsf) == msdr.STATUS_ARGUMENT_ERROR
    assert lib.msdr_chain_set_prefilter(None, C.c_uint32(1), C.c_uint32(0), None) == msdr.STATUS_ARGUMENT_ERROR          # (turning off needs a chain too)
    assert lib.msdr_chain_get_prefilter(None, C.byref(d), C.byref(n)) == msdr.STATUS_ARGUMENT_ERROR and (d.value, n.value) == (7, 9)


def test_the_flavour_bit_is_an_enumerator_and_the_binding_mirrors_the_header():
    m = re.search(r"enum\s*\{\s*MSDR_FLAVOUR_PREFILTER\s*=\s*(0x[0-9a-fA-F]+)u\s*\}\s*;", CODE)
    assert m and int(m.group(1), 16) == 0x8000000 == msdr.FLAVOUR_PREFILTER
    assert not re.search(r"#define\s+MSDR_FLAVOUR_PREFILTER", HDR)
    others = {n: int(v, 0) for n, v in re.findall(r"MSDR_(FLAVOUR_[A-Z_0-9]+)\s*=?\s+(0x[0-9a-fA-F]+)u", CODE) if n != "FLAVOUR_PREFILTER"}
    assert len(others) >= 20 and all(v != 0x8000000 for v in others.values()), others


def test_the_host_node_sets_the_prefilter_and_its_readers_follow_the_product_of_the_factors():
    assert re.search(r"int setPrefilter\(uint32_t D1, const int16_t \*taps, uint32_t n\) \{ return chain \? msdr_chain_set_prefilter\(chain, D1, n, taps\)", NODES)
    assert re.search(r"int setPrefilter\(uint32_t D1, const float \*taps, uint32_t n\) \{ return chain \? msdr_chain_set_prefilter_f32\(chain, D1, n, taps\)", NODES)
    body = NODES[NODES.index("int rateDivisor("):]
    assert "msdr_chain_get_decimation(chain, &D)" in body[:400] and "msdr_chain_get_prefilter(chain, &D1, nullptr)" in body[:400] and "*div = D * D1;" in body[:400]
    for reader in ("int readLevels(", "int readIq("):
        b = NODES[NODES.index(reader):]
        b = b[:b.index("\n    }\n")]
        assert "rateDivisor(&D)" in b and "msdr_chain_get_decimation" not in b, reader
