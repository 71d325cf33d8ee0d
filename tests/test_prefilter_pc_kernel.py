"""The two-stage decimating chain kernels (minimal-sdr_amd/csrc/msdr_chain_pre.hiph).  The translation unit is compiled to gfx950 assembly with
the product's flags and the code-object metadata is read: the plain body and the full twin (METER, IQ and GAIN compiled in) of both
arithmetics are there by name for channels per wave 1, 2, 4 and every read width of the second stage -- 42 kernels -- without scratch, without
vector spills and without static LDS.  The plain bodies are held to the register budget their launch bounds give them, the full twins to
that of three waves per SIMD.  Metadata fields only; no GPU needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minimal-sdr_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
# the product's flags (minimal-sdr_amd/Makefile: HIPFLAGS)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fwrapv", "-fno-slp-vectorize"]
CPWS = (1, 2, 4)
KERNELS = (["chain_q15pcn2_%skernelILi%dELi%dEE" % (f, c, al) for f in ("", "full_") for c in CPWS for al in (0, 1, 2, 4)] +
           ["chain_f32pcn2_%skernelILi%dELi%dEE" % (f, c, al) for f in ("", "full_") for c in CPWS for al in (1, 2, 4)])


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """mangled kernel name -> its block of amdhsa.kernels"""
    d = str(tmp_path_factory.mktemp("prepc"))
    s = os.path.join(d, "msdr_chain_pre.s")
    p = subprocess.run([HIPCC] + FLAGS + ["-S", "--cuda-device-only", "-o", s, os.path.join(CSRC, "msdr_chain_pre.hip")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    with open(s) as f:
        asm = f.read()
    found = {}
    for block in re.split(r"\n\s+- \.agpr_count:", "\n" + asm[asm.index("amdhsa.kernels"):])[1:]:
        block = ".agpr_count:" + block
        found[re.search(r"\.name:\s+(\S+)", block).group(1)] = block
    return found


def _field(block, name):
    return int(re.search(r"\.%s:\s+(\d+)" % name, block).group(1))


def test_every_instantiation_is_present_without_scratch_vector_spills_or_static_lds(kernels):
    assert len(KERNELS) == 24 + 18
    for needle in KERNELS:
        hits = [k for k in kernels if needle in k]
        assert len(hits) == 1, (needle, hits)
        name, block = hits[0], kernels[hits[0]]
        assert _field(block, "private_segment_fixed_size") == 0, name
        assert _field(block, "vgpr_spill_count") == 0, name
        assert _field(block, "group_segment_fixed_size") == 0, name
        # 512 vector registers per SIMD lane: three waves per SIMD (the full twins' attribute, and what 256 threads need at least) leave 168
        assert _field(block, "vgpr_count") + _field(block, "agpr_count") <= 168, (name, _field(block, "vgpr_count"), _field(block, "agpr_count"))


def test_the_unit_adds_no_other_chain_kernel(kernels):
    assert sorted(k for k in kernels if "chain_" in k) == sorted(k for k in kernels if any(n in k for n in KERNELS))
