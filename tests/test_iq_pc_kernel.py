"""The IQ flavours of the phase-accumulator chain kernels (msdr_chain_iq.hiph: pc_frame / pf_frame / the decimating pair with IQ, alone and beside
METER).  The two translation units are compiled to gfx950 assembly with the product's flags and the code-object metadata is read: every
`_iq_` and `_iq_meter_` instantiation is there by name -- channels per wave 1, 2, 4, every read width of the decimating pair -- within 128
vector registers, without scratch, spills or static LDS (the pairs are packed in registers: the launch's dynamic LDS is the plain kernel's).
Metadata fields only; no GPU needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minimal-sdr_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
# the product's flags (minimal-sdr_amd/Makefile: HIPFLAGS)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fwrapv", "-fno-slp-vectorize"]
UNITS = ("msdr_chain_ncopc", "msdr_chain_decpc")
CPWS = (1, 2, 4)
TAPPED = (["chain_%spcn_%s_kernelILi%dEE" % (a, f, c) for a in ("q15", "f32") for f in ("iq", "iq_meter") for c in CPWS] +
          ["chain_q15pcnd_%s_kernelILi%dELi%dEE" % (f, c, al) for f in ("iq", "iq_meter") for c in CPWS for al in (0, 1, 2, 4)] +
          ["chain_f32pcnd_%s_kernelILi%dELi%dEE" % (f, c, al) for f in ("iq", "iq_meter") for c in CPWS for al in (1, 2, 4)])
# the kernels these units had before: each still found exactly once, so no new name contains an old one
BEFORE = (["chain_%spcn_%skernelILi%dEE" % (a, f, c) for a in ("q15", "f32") for f in ("", "meter_") for c in CPWS] +
          ["chain_q15pcnd_%skernelILi%dELi%dEE" % (f, c, al) for f in ("", "meter_") for c in CPWS for al in (0, 1, 2, 4)] +
          ["chain_f32pcnd_%skernelILi%dELi%dEE" % (f, c, al) for f in ("", "meter_") for c in CPWS for al in (1, 2, 4)])


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """mangled kernel name -> its block of amdhsa.kernels, over the two units (compiled side by side)"""
    d = str(tmp_path_factory.mktemp("iqpc"))
    procs = [(u, subprocess.Popen([HIPCC] + FLAGS + ["-S", "--cuda-device-only", "-o", os.path.join(d, u + ".s"), os.path.join(CSRC, u + ".hip")],
                                  stdout=subprocess.PIPE, stderr=subprocess.PIPE)) for u in UNITS]
    found = {}
    for u, p in procs:
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, (u, err.decode()[-2000:])
        with open(os.path.join(d, u + ".s")) as f:
            asm = f.read()
        for block in re.split(r"\n\s+- \.agpr_count:", "\n" + asm[asm.index("amdhsa.kernels"):])[1:]:
            block = ".agpr_count:" + block
            found[re.search(r"\.name:\s+(\S+)", block).group(1)] = block
    return found


def _one(kernels, needle):
    hits = [k for k in kernels if needle in k]
    assert len(hits) == 1, (needle, hits)
    return hits[0], kernels[hits[0]]


def _field(block, name):
    return int(re.search(r"\.%s:\s+(\d+)" % name, block).group(1))


def test_every_iq_instantiation_is_present_within_the_register_file_and_without_scratch_or_static_lds(kernels):
    assert len(TAPPED) == 12 + 24 + 18
    for needle in TAPPED:
        name, block = _one(kernels, needle)
        assert _field(block, "vgpr_count") + _field(block, "agpr_count") <= 128, (name, _field(block, "vgpr_count"), _field(block, "agpr_count"))
        assert _field(block, "private_segment_fixed_size") == 0, name
        assert _field(block, "vgpr_spill_count") == 0, name          # (nothing goes to memory; scalar registers parked in lanes of a vector
        #                                                               register, as in the decimating Q15 kernels' metered twins, are inside vgpr_count)
        assert _field(block, "group_segment_fixed_size") == 0, name


def test_every_kernel_of_before_is_still_found_exactly_once(kernels):
    assert len(BEFORE) == 12 + 24 + 18
    for needle in BEFORE:
        _one(kernels, needle)
