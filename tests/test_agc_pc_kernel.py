"""The gain twins of the phase-accumulator chain kernels (msdr_chain_gain.hiph: the frames of msdr_chain_q15pc.hiph / msdr_chain_f32pc.hiph /
msdr_chain_decpc.hiph with GAIN, real and complex input).  The two new translation units are compiled to gfx950 assembly with the product's
flags and the code-object metadata is read: every twin is there by name -- ONE per family, input, channels per wave and read width, the
superset of the plain, metered and I/Q bodies -- within the 168 vector registers of its own occupancy attribute (three waves per SIMD),
without scratch, vector spills or static LDS.  Metadata fields only; no GPU needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minimal-sdr_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
# the product's flags (minimal-sdr_amd/Makefile: HIPFLAGS)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fwrapv", "-fno-slp-vectorize"]
UNITS = ("msdr_chain_gncopc", "msdr_chain_gdecpc")
CPWS = (1, 2, 4)
INPUTS = ("", "cx_")
TWINS = (["chain_%spcn_%sgain_kernelILi%dEE" % (a, i, c) for a in ("q15", "f32") for i in INPUTS for c in CPWS] +
         ["chain_q15pcnd_%sgain_kernelILi%dELi%dEE" % (i, c, al) for i in INPUTS for c in CPWS for al in (0, 1, 2, 4)] +
         ["chain_f32pcnd_%sgain_kernelILi%dELi%dEE" % (i, c, al) for i in INPUTS for c in CPWS for al in (1, 2, 4)])
# the existing kernels' names: none of them may be found inside a new name (the sibling tests look kernels up by substring)
FLAVOURS = ("", "meter_", "iq_", "iq_meter_")
OLD = ["chain_%s%s_%s%skernel" % (a, fam, i, f) for a in ("q15", "f32") for fam in ("pcn", "pcnd") for i in INPUTS for f in FLAVOURS]
VGPRS = 168          # 512 / 3, in allocation granules of 8: what amdgpu_waves_per_eu(3) leaves a wave


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """mangled kernel name -> its block of amdhsa.kernels, over the two units (compiled side by side)"""
    d = str(tmp_path_factory.mktemp("gainpc"))
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


def test_every_gain_twin_is_present_within_its_registers_and_without_scratch_or_static_lds(kernels):
    assert len(TWINS) == 12 + 24 + 18
    for needle in TWINS:
        hits = [k for k in kernels if needle in k]
        assert len(hits) == 1, (needle, hits)
        name, block = hits[0], kernels[hits[0]]
        assert _field(block, "vgpr_count") + _field(block, "agpr_count") <= VGPRS, (name, _field(block, "vgpr_count"), _field(block, "agpr_count"))
        assert _field(block, "private_segment_fixed_size") == 0, name
        assert _field(block, "vgpr_spill_count") == 0, name
        assert _field(block, "group_segment_fixed_size") == 0, name


def test_one_twin_per_family_and_geometry_and_no_new_name_contains_an_old_one(kernels):
    chain = [k for k in kernels if "chain_" in k]
    assert len(chain) == len(TWINS), sorted(set(chain) - {k for k in chain if any(t in k for t in TWINS)})
    for k in chain:
        assert not any(o in k for o in OLD), k
