"""The metered flavours of the per-receiver chain kernels (msdr_chain_meter.hiph: pc_frame / pf_frame / the decimating pair with METER).  The
five translation units are compiled to gfx950 assembly with the product's flags and the code-object metadata is read: every metered
instantiation is there by name -- channels per wave 1, 2, 4, both mixers of chain_f32pc, every read width of the decimating pair -- within 128
vector registers, without scratch, spills or static LDS (the meter lives in registers: the launch's dynamic LDS is the unmetered kernel's), and
every unmetered instantiation is still there beside it.  No GPU needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minimal-sdr_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
# the product's flags (minimal-sdr_amd/Makefile: HIPFLAGS)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fwrapv", "-fno-slp-vectorize"]
UNITS = ("msdr_chain_q15pc", "msdr_chain_f32pc", "msdr_chain_oscpc", "msdr_chain_ncopc", "msdr_chain_decpc")
CPWS = (1, 2, 4)
METERED = (["chain_q15pc_meter_kernelILi%dEE" % c for c in CPWS] + ["chain_f32pc_meter_kernelILi%dELb%dEE" % (c, f) for c in CPWS for f in (0, 1)] +
           ["chain_%spc%s_meter_kernelILi%dEE" % (a, o, c) for a in ("q15", "f32") for o in ("o", "n") for c in CPWS] +
           ["chain_q15pcnd_meter_kernelILi%dELi%dEE" % (c, al) for c in CPWS for al in (0, 1, 2, 4)] +
           ["chain_f32pcnd_meter_kernelILi%dELi%dEE" % (c, al) for c in CPWS for al in (1, 2, 4)])
UNMETERED = (["chain_q15pc_kernelILi%dELb%dEE" % (c, f) for c in CPWS for f in (0, 1)] +
             ["chain_f32pc_kernelILi%dELb%dELb%dEE" % (c, f, s) for c in CPWS for f, s in ((0, 0), (0, 1), (1, 0))] +
             ["chain_%spc%s_kernelILi%dEE" % (a, o, c) for a in ("q15", "f32") for o in ("o", "n") for c in CPWS] +
             ["chain_q15pcnd_kernelILi%dELi%dEE" % (c, al) for c in CPWS for al in (0, 1, 2, 4)] +
             ["chain_f32pcnd_kernelILi%dELi%dEE" % (c, al) for c in CPWS for al in (1, 2, 4)])


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """mangled kernel name -> its block of amdhsa.kernels, over the five units (compiled side by side)"""
    d = str(tmp_path_factory.mktemp("meterpc"))
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


def test_every_metered_instantiation_is_present_within_the_register_file_and_without_static_lds(kernels):
    assert len(METERED) == 3 + 6 + 12 + 12 + 9
    for needle in METERED:
        name, block = _one(kernels, needle)
        vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", block).group(1))
        agpr = int(re.search(r"\.agpr_count:\s+(\d+)", block).group(1))
        assert vgpr + agpr <= 128, (name, vgpr, agpr)
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)) == 0, name
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1)) == 0, name
        assert int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1)) == 0, name


def test_every_unmetered_instantiation_is_still_present(kernels):
    assert len(UNMETERED) == 6 + 9 + 12 + 12 + 9
    for needle in UNMETERED:
        _one(kernels, needle)
