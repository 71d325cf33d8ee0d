"""biquad_teensy_pc_kernel (minimal-sdr_amd/csrc/msdr_biquad_pc.hiph): the AudioFilterBiquad node kernel whose coefficients and stage count
are per lane.  Its coefficients sit in vector registers for the whole call; a spill would put scratch traffic into the sample loop, whose
dependent chain is the floor of the node pass.  The translation unit is compiled to assembly here and every instantiation is checked: present
by name, no scratch instruction, at most 128 vector registers (read from the compiler's kernel metadata).  Also the host side of the two
new setters: declared, exported, and refusing a malformed array before any library call.  No GPU needed."""
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
INSTANCES = ("biquad_teensy_pc_kernelILi1E", "biquad_teensy_pc_kernelILi2E")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("pc")), "msdr_biquad_pc.s")
    subprocess.run([HIPCC] + FLAGS + ["-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "msdr_biquad_pc.hip")], check=True,
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
        assert sum(1 for i in ins if i.startswith("v_dot2")) >= 8, name                 # the right function: tbq_step's packed products
        assert sum(1 for i in ins if i.startswith("ds_read_b128") or i.startswith("ds_load_b128")) >= 1, name
        scratch = [i for i in ins if "scratch_" in i]
        assert not scratch, (name, scratch[:4])


def test_every_instantiation_keeps_to_128_vector_registers(asm):
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


def test_the_new_setters_are_declared_in_the_header():
    with open(os.path.join(ROOT, "include", "msdr.h")) as f:
        h = f.read()
    for sym in ("msdr_biquad_q15_set_coefficients_channels", "msdr_chain_set_node_coefficients_channels"):
        assert re.search(r"^int %s\(" % sym, h, re.M), sym


def test_python_setters_refuse_a_count_by_4_array_before_any_library_call():
    sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
    import msdr
    b = msdr.BiquadQ15.__new__(msdr.BiquadQ15)            # objects that never reach the library: no ctx, no handle
    c = msdr.Chain.__new__(msdr.Chain)
    try:
        for bad in (np.zeros((3, 4), np.int32), np.zeros(5, np.int32), np.zeros((2, 5, 1), np.int32), np.zeros((3, 6), np.int32)):
            with pytest.raises(ValueError):
                b.set_coefficients_channels(0, 0, bad)
            with pytest.raises(ValueError):
                c.set_node_coefficients_channels(1, 0, 0, bad)
        with pytest.raises(AttributeError):                # a well-formed array gets as far as the (missing) library handle
            b.set_coefficients_channels(0, 0, np.zeros((3, 5), np.int32))
    finally:
        b.h = None
        c.h = None
