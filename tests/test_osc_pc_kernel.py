"""chain_q15pco_kernel / chain_f32pco_kernel (minimal-sdr_amd/csrc/msdr_chain_oscpc.hiph): the chain kernels whose oscillator operand is per
channel.  The translation unit is compiled to assembly here and every instantiation is checked: present by name, the Q15 products are
v_dot2, the oscillator row goes through LDS, no scratch, at most 128 vector registers, no private segment and no spills (the compiler's
kernel metadata).  Also the host side of the new call: declared in include/msdr.h, exported by libmsdr.so, the config struct's size and
the flavour bit mirrored in the Python binding, malformed arrays refused before any library call.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minimal-sdr_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
# the product's flags (minimal-sdr_amd/Makefile: HIPFLAGS)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fwrapv", "-fno-slp-vectorize"]
Q15 = tuple("chain_q15pco_kernelILi%dEE" % cpw for cpw in (1, 2, 4))
F32 = tuple("chain_f32pco_kernelILi%dEE" % cpw for cpw in (1, 2, 4))
INSTANCES = Q15 + F32


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("oscpc")), "msdr_chain_oscpc.s")
    subprocess.run([HIPCC] + FLAGS + ["-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "msdr_chain_oscpc.hip")], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    with open(out) as f:
        return f.read()


def _body(text, needle):
    """the instructions between `<mangled name>:` and the end of the function (basic blocks may follow its s_endpgm)"""
    m = re.search(r"^(\S*%s\S*):" % re.escape(needle), text, re.M)
    assert m, "no kernel %s in the translation unit" % needle
    start = m.end()
    end = text.index("\n.Lfunc_end", text.index("s_endpgm", start))
    return m.group(1), [ln.strip() for ln in text[start:end].splitlines() if ln.strip() and not ln.strip().startswith((";", "."))]


def _lds_writes(ins):
    return sum(1 for i in ins if i.startswith("ds_write") or i.startswith("ds_store"))


def test_every_instantiation_is_present_with_its_products_and_without_scratch_traffic(asm):
    for needle in INSTANCES:
        name, ins = _body(asm, needle)
        if needle in Q15:
            assert sum(1 for i in ins if i.startswith("v_dot2")) >= 64, name          # one step = 8 taps x 8 outputs per filter
        assert not [i for i in ins if "scratch_" in i], name


def test_the_oscillator_row_goes_through_lds(asm):
    """The row is written to LDS beside the tap rows and the window, and the mix READS it entry by entry: one dword (Q15: the packed pair) or
    two (F32: a float2) per read.  The FIR phase reads whole 16-byte slots, and chain_q15pc_kernel / chain_f32pc_kernel, whose pairs come
    from global memory, have no narrower LDS read than that."""
    for needle in INSTANCES:
        name, ins = _body(asm, needle)
        reads = [i.split()[0] for i in ins if i.startswith("ds_read") or i.startswith("ds_load")]
        assert any(r.endswith("_b128") for r in reads), name
        narrow = "_b32" if needle in Q15 else "_b64"
        assert any(r.endswith(narrow) for r in reads), (name, sorted(set(reads)))
        assert _lds_writes(ins) >= 3, (name, "tap rows, oscillator row, window")


def test_every_instantiation_keeps_to_128_vector_registers_and_zero_scratch(asm):
    meta = asm[asm.index("amdhsa.kernels"):]
    seen = 0
    for block in re.split(r"\n\s+- \.agpr_count:", "\n" + meta)[1:]:
        block = ".agpr_count:" + block
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        if not any(n in name for n in INSTANCES):
            continue
        seen += 1
        vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1))
        agpr = int(re.search(r"\.agpr_count:\s+(\d+)", block).group(1))
        assert vgpr + agpr <= 128, (name, vgpr, agpr)
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)) == 0, name
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1)) == 0, name
    assert seen == len(INSTANCES), seen


def test_the_new_call_is_declared_exported_and_mirrored(tmp_path):
    with open(os.path.join(ROOT, "include", "msdr.h")) as f:
        h = f.read()
    assert re.search(r"^int msdr_chain_set_osc_channels\(", h, re.M)
    assert re.search(r"^enum \{ MSDR_FLAVOUR_OSC_PC = 0x20000u \};", h, re.M)           # an enumerator: tests/test_abi.py counts the macros
    lib = os.path.join(ROOT, "minimal-sdr_amd", "lib", "libmsdr.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    assert re.search(r" T msdr_chain_set_osc_channels$", out, re.M)
    src = os.path.join(str(tmp_path), "size.c")
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include "msdr.h"\nint main(void) { printf("%zu %u\\n", sizeof(msdr_chain_config), (unsigned)MSDR_FLAVOUR_OSC_PC); return 0; }\n')
    exe = os.path.join(str(tmp_path), "size")
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), "-o", exe, src])
    size, bit = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
    import msdr
    assert int(size) == C.sizeof(msdr.ChainConfig) == 264          # the struct as every earlier build laid it out (LP64)
    assert int(bit) == msdr.FLAVOUR_OSC_PC == 0x20000
    assert not msdr.FLAVOUR_OSC_PC & (msdr.FLAVOUR_TAPS_PC | msdr.FLAVOUR_CASCADE_PC | 0x7FFF)


def test_set_osc_channels_refuses_malformed_arrays_before_any_library_call():
    sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
    import msdr
    c = msdr.Chain.__new__(msdr.Chain)                    # an object that never reaches the library: no ctx, no handle
    c.osc_len = 128
    try:
        for arith, dt, other in ((msdr.ARITH_Q15, np.int16, np.float32), (msdr.ARITH_F32, np.float32, np.complex64)):
            c.arith = arith
            good = np.zeros((3, 128), dt)
            for bad in (np.zeros((3, 100), dt), np.zeros(128, dt), np.zeros((2, 128, 1), dt), np.zeros((3, 128), other)):
                with pytest.raises(ValueError):
                    c.set_osc_channels(0, bad, good)
                with pytest.raises(ValueError):
                    c.set_osc_channels(0, good, bad)
            with pytest.raises(ValueError):               # both well-formed, not the same shape
                c.set_osc_channels(0, good, np.zeros((2, 128), dt))
            with pytest.raises(AttributeError):           # well-formed arrays get as far as the (missing) library handle
                c.set_osc_channels(0, good, good)
        c.arith = msdr.ARITH_Q15
        with pytest.raises(ValueError):                   # not an int16
            c.set_osc_channels(0, np.full((1, 128), 40000, np.int32), np.zeros((1, 128), np.int32))
    finally:
        c.h = None
