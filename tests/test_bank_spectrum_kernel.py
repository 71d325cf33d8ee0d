"""The 64-point complex FFT kernels of the per-receiver spectrum display (msdr_bank_spectrum.hiph / msdr_bank_spectrum.hip).  The new
translation unit is compiled to gfx950 assembly with the product's flags and the code-object metadata is read: both kernels are there by
name, 256 threads per workgroup (16 transforms of 16 lanes), without scratch or spills, with their static LDS -- 48 twiddle pairs and 16
transforms of 64 pairs at a pitch of 68 dwords (Q15: 4 736 bytes) or 80 float pairs (F32: 10 624 bytes) -- and within 64 vector registers,
so that eight waves per SIMD stay possible (profiles/bank_spectrum/README.md records the counts: 48 and 55).  Metadata fields only; no GPU needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minimal-sdr_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
# the product's flags (minimal-sdr_amd/Makefile: HIPFLAGS)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fwrapv", "-fno-slp-vectorize"]
UNIT = "msdr_bank_spectrum"
# kernel -> static LDS bytes
KERNELS = {"bank_cfft64_q15_kernel": 48 * 8 + 16 * 68 * 4, "bank_cfft64_f32_kernel": 48 * 8 + 16 * 80 * 8}
VGPRS = 64
THREADS = 256


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """mangled kernel name -> its block of amdhsa.kernels"""
    d = str(tmp_path_factory.mktemp("bankspectrum"))
    p = subprocess.run([HIPCC] + FLAGS + ["-S", "--cuda-device-only", "-o", os.path.join(d, UNIT + ".s"), os.path.join(CSRC, UNIT + ".hip")],
                       capture_output=True, timeout=900)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    with open(os.path.join(d, UNIT + ".s")) as f:
        asm = f.read()
    found = {}
    for block in re.split(r"\n\s+- \.agpr_count:", "\n" + asm[asm.index("amdhsa.kernels"):])[1:]:
        block = ".agpr_count:" + block
        found[re.search(r"\.name:\s+(\S+)", block).group(1)] = block
    return found


def _field(block, name):
    return int(re.search(r"\.%s:\s+(\d+)" % name, block).group(1))


def test_both_kernels_are_present_without_scratch_or_spills(kernels):
    for needle, lds in KERNELS.items():
        hits = [k for k in kernels if needle in k]
        assert len(hits) == 1, (needle, hits)
        name, block = hits[0], kernels[hits[0]]
        assert _field(block, "private_segment_fixed_size") == 0, name
        assert _field(block, "vgpr_spill_count") == 0 and _field(block, "sgpr_spill_count") == 0, name
        assert _field(block, "agpr_count") == 0, name
        assert _field(block, "vgpr_count") <= VGPRS, (name, _field(block, "vgpr_count"))
        assert _field(block, "group_segment_fixed_size") == lds, (name, _field(block, "group_segment_fixed_size"))
        assert _field(block, "max_flat_workgroup_size") == THREADS, name


def test_no_other_kernel_of_the_unit_carries_a_bank_name(kernels):
    assert sorted(k for k in kernels if "bank_" in k) == sorted(k for k in kernels if any(n in k for n in KERNELS))


def test_the_unit_is_one_of_the_librarys_kernel_objects():
    with open(os.path.join(ROOT, "minimal-sdr_amd", "Makefile")) as f:
        assert "$(OUT)/" + UNIT + ".o" in f.read()
