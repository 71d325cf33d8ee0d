"""The complex-input twins of the phase-accumulator chain kernels (msdr_chain_cxpc.hiph: the frames of msdr_chain_ncopc.hiph / msdr_chain_decpc.hiph
with the oscillator policies PcOscPhaseCx / PfOscPhaseCx).  The two new translation units are compiled to gfx950 assembly with the product's
flags and the code-object metadata is read: every `cx` instantiation is there by name -- plain, meter, iq, iq_meter; channels per wave 1, 2, 4;
every read width of the decimating pair -- within 128 vector registers, without scratch, spills or static LDS (the four products and two sums
of the complex mix live during staging only).  Metadata fields only; no GPU needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minimal-sdr_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
# the product's flags (minimal-sdr_amd/Makefile: HIPFLAGS)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fwrapv", "-fno-slp-vectorize"]
UNITS = ("msdr_chain_cxncopc", "msdr_chain_cxdecpc")
CPWS = (1, 2, 4)
FLAVOURS = ("", "meter_", "iq_", "iq_meter_")
TWINS = (["chain_%spcn_cx_%skernelILi%dEE" % (a, f, c) for a in ("q15", "f32") for f in FLAVOURS for c in CPWS] +
         ["chain_q15pcnd_cx_%skernelILi%dELi%dEE" % (f, c, al) for f in FLAVOURS for c in CPWS for al in (0, 1, 2, 4)] +
         ["chain_f32pcnd_cx_%skernelILi%dELi%dEE" % (f, c, al) for f in FLAVOURS for c in CPWS for al in (1, 2, 4)])
# the real kernels' names: none of them may be found inside a new name (the sibling tests look kernels up by substring)
REAL = (["chain_%spcn_%skernel" % (a, f) for a in ("q15", "f32") for f in FLAVOURS] + ["chain_%spcnd_%skernel" % (a, f) for a in ("q15", "f32") for f in FLAVOURS])


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """mangled kernel name -> its block of amdhsa.kernels, over the two units (compiled side by side)"""
    d = str(tmp_path_factory.mktemp("cxpc"))
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


def _field(block, name):
    return int(re.search(r"\.%s:\s+(\d+)" % name, block).group(1))


def test_every_cx_instantiation_is_present_within_the_register_file_and_without_scratch_or_static_lds(kernels):
    assert len(TWINS) == 24 + 48 + 36
    for needle in TWINS:
        hits = [k for k in kernels if needle in k]
        assert len(hits) == 1, (needle, hits)
        name, block = hits[0], kernels[hits[0]]
        assert _field(block, "vgpr_count") + _field(block, "agpr_count") <= 128, (name, _field(block, "vgpr_count"), _field(block, "agpr_count"))
        assert _field(block, "private_segment_fixed_size") == 0, name
        assert _field(block, "vgpr_spill_count") == 0, name
        assert _field(block, "group_segment_fixed_size") == 0, name


def test_no_new_name_contains_an_old_one(kernels):
    chain = [k for k in kernels if "chain_" in k]
    assert len(chain) == len(TWINS), sorted(set(chain) - {k for k in chain if any(t in k for t in TWINS)})
    for k in chain:
        assert not any(r in k for r in REAL), k
