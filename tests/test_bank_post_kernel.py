"""The PLL kernels behind the down-converter bank (msdr_bank_post.hiph / msdr_bank_post.hip).  The new translation unit is compiled to gfx950
assembly with the product's flags and the code-object metadata is read: both kernels are there by name, one wave per workgroup, without
scratch or vector spills, with the slab's static LDS (64 rows of 65 pairs: 16 640 bytes of dwords, 33 280 of float pairs) and within 128
vector registers (profiles/bank_post/README.md records the counts: 94 and 98).  Metadata fields only; no GPU needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minimal-sdr_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
# the product's flags (minimal-sdr_amd/Makefile: HIPFLAGS)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fwrapv", "-fno-slp-vectorize"]
UNIT = "msdr_bank_post"
# kernel -> static LDS bytes
KERNELS = {"bank_pll_q15_kernel": 64 * 65 * 4, "bank_pll_f32_kernel": 64 * 65 * 8}
VGPRS = 128          # four one-wave workgroups per SIMD stay possible; both kernels are far below it


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """mangled kernel name -> its block of amdhsa.kernels"""
    d = str(tmp_path_factory.mktemp("bankpost"))
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
        assert _field(block, "max_flat_workgroup_size") == 64, name


def test_no_other_kernel_of_the_unit_carries_a_bank_name(kernels):
    assert sorted(k for k in kernels if "bank_" in k) == sorted(k for k in kernels if any(n in k for n in KERNELS))
