"""chain_q15pc_kernel (minimal-sdr_amd/csrc/msdr_chain_q15pc.hiph): the Q15 chain kernel whose FIR coefficient operand is per channel.
The translation unit is compiled to assembly here and every instantiation is checked: present by name, its products are v_dot2_i32_i16,
no scratch, at most 128 vector registers (read from the compiler's kernel metadata).  Also the host side of the new calls: declared in
include/msdr.h, exported by libmsdr.so, the public constants unchanged, malformed arrays refused before any library call.  No GPU needed."""
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
INSTANCES = tuple("chain_q15pc_kernelILi%dELb%dEE" % (cpw, fir) for cpw in (1, 2, 4) for fir in (0, 1))
SYMBOLS = ("msdr_chain_set_taps_channels", "msdr_fir_q15_set_coeffs_channels")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("pc")), "msdr_chain_q15pc.s")
    subprocess.run([HIPCC] + FLAGS + ["-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "msdr_chain_q15pc.hip")], check=True,
                   stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    with open(out) as f:
        return f.read()


def _body(text, needle):
    """the instructions between `<mangled name>:` and its s_endpgm"""
    m = re.search(r"^(\S*%s\S*):" % re.escape(needle), text, re.M)
    assert m, "no kernel %s in the translation unit" % needle
    start = m.end()
    end = text.index("s_endpgm", start)
    return m.group(1), [ln.strip() for ln in text[start:end].splitlines() if ln.strip() and not ln.strip().startswith((";", "."))]


def test_every_instantiation_is_present_without_scratch_traffic(asm):
    for needle in INSTANCES:
        name, ins = _body(asm, needle)
        assert sum(1 for i in ins if i.startswith("v_dot2")) >= 64, name              # one step = 8 taps x 8 outputs per filter
        assert sum(1 for i in ins if i.startswith("ds_read_b128") or i.startswith("ds_load_b128")) >= 4, name
        assert not [i for i in ins if "scratch_" in i], name


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


def test_the_new_calls_are_declared_and_the_public_constants_are_unchanged():
    with open(os.path.join(ROOT, "include", "msdr.h")) as f:
        h = f.read()
    for sym in SYMBOLS:
        assert re.search(r"^int %s\(" % sym, h, re.M), sym
    assert re.search(r"^#define MSDR_MAX_TAPSETS 8\s*$", h, re.M)


def test_the_library_exports_the_new_calls_and_the_config_struct_keeps_its_size(tmp_path):
    lib = os.path.join(ROOT, "minimal-sdr_amd", "lib", "libmsdr.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    for sym in SYMBOLS:
        assert re.search(r" T %s$" % sym, out, re.M), sym
    src = os.path.join(str(tmp_path), "size.c")
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include "msdr.h"\nint main(void) { printf("%zu %d\\n", sizeof(msdr_chain_config), MSDR_MAX_TAPSETS); return 0; }\n')
    exe = os.path.join(str(tmp_path), "size")
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), "-o", exe, src])
    size, sets = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
    import msdr
    assert int(sets) == 8
    assert int(size) == C.sizeof(msdr.ChainConfig) == 264          # the struct as every earlier build laid it out (LP64)


def test_python_setters_refuse_malformed_arrays_before_any_library_call():
    sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
    import msdr
    f = msdr.FirQ15.__new__(msdr.FirQ15)                  # objects that never reach the library: no ctx, no handle
    c = msdr.Chain.__new__(msdr.Chain)
    f.ntaps = c.ntaps = 102
    try:
        for bad in (np.zeros((3, 100), np.int16), np.zeros(102, np.int16), np.zeros((2, 102, 1), np.int16)):
            with pytest.raises(ValueError):
                f.set_coeffs_channels(0, bad)
            with pytest.raises(ValueError):
                c.set_taps_channels(0, bad)
        with pytest.raises(ValueError):
            c.set_taps_channels(0, np.zeros((3, 102), np.int16), np.zeros((2, 102), np.int16))
        with pytest.raises(AttributeError):                # a well-formed array gets as far as the (missing) library handle
            f.set_coeffs_channels(0, np.zeros((3, 102), np.int16))
    finally:
        f.h = None
        c.h = None
