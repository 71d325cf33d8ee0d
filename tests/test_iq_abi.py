"""The host side of the baseband I/Q output (msdr_chain_set_iq_out / msdr_chain_get_iq_out, MSDR_FLAVOUR_IQ_OUT): declared in include/msdr.h,
exported by libmsdr.so, the flavour bit an enumerator that collides with no other, msdr_chain_config as every earlier build laid it out, the
Python mirror, and a NULL chain refused.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
import msdr  # noqa: E402


def test_the_calls_are_declared_exported_and_mirrored(tmp_path):
    with open(os.path.join(ROOT, "include", "msdr.h")) as f:
        h = f.read()
    for decl in (r"^int msdr_chain_set_iq_out\(msdr_chain \*chain, void \*d_iq, uint64_t pitch\);",
                 r"^int msdr_chain_get_iq_out\(msdr_chain \*chain, void \*\*d_iq, uint64_t \*pitch\);"):
        assert re.search(decl, h, re.M), decl
    assert re.search(r"^enum \{ MSDR_FLAVOUR_IQ_OUT = 0x400000u \};", h, re.M)          # an enumerator: tests/test_abi.py counts the macros
    assert not re.search(r"#\s*define\s+MSDR_FLAVOUR_IQ_OUT", h)
    lib = os.path.join(ROOT, "minimal-sdr_amd", "lib", "libmsdr.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    for sym in ("msdr_chain_set_iq_out", "msdr_chain_get_iq_out"):
        assert re.search(r" T %s$" % sym, out, re.M), sym
    others = sorted(set(re.findall(r"MSDR_FLAVOUR_[A-Z0-9_]+", h)) - {"MSDR_FLAVOUR_IQ_OUT", "MSDR_FLAVOUR_FOLD_PERIOD_SHIFT", "MSDR_FLAVOUR_FOLD_PERIOD"})
    assert len(others) >= 18 and "MSDR_FLAVOUR_METER" in others, others
    src = os.path.join(str(tmp_path), "size.c")
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include "msdr.h"\nint main(void) { printf("%zu %u %u\\n", sizeof(msdr_chain_config), (unsigned)MSDR_FLAVOUR_IQ_OUT,\n'
                '    (unsigned)(' + " | ".join(others) + ' | (7u << MSDR_FLAVOUR_FOLD_PERIOD_SHIFT))); return 0; }\n')
    exe = os.path.join(str(tmp_path), "size")
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), "-o", exe, src])
    size, bit, rest = (int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split())
    assert size == C.sizeof(msdr.ChainConfig) == 264          # the struct as every earlier build laid it out (LP64)
    assert bit == msdr.FLAVOUR_IQ_OUT == 0x400000
    assert not bit & rest, hex(rest)                         # disjoint from every other flavour bit and from the fold period's field
    assert callable(msdr.Chain.set_iq_out) and callable(msdr.Chain.iq_out)
    assert msdr.load_library().msdr_chain_set_iq_out.argtypes[2] is C.c_uint64          # the pitch travels as 64 bits


def test_a_null_chain_is_an_argument_error():
    lib = msdr.load_library()
    p, pitch = C.c_void_p(), C.c_uint64()
    assert lib.msdr_chain_set_iq_out(None, None, 0) == msdr.STATUS_ARGUMENT_ERROR
    assert lib.msdr_chain_set_iq_out(None, C.c_void_p(4096), 8) == msdr.STATUS_ARGUMENT_ERROR
    assert lib.msdr_chain_get_iq_out(None, C.byref(p), C.byref(pitch)) == msdr.STATUS_ARGUMENT_ERROR
    assert lib.msdr_chain_get_iq_out(None, None, None) == msdr.STATUS_ARGUMENT_ERROR
