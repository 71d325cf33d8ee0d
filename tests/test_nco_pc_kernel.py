"""chain_q15pcn_kernel / chain_f32pcn_kernel (minimal-sdr_amd/csrc/msdr_chain_ncopc.hiph): the per-receiver chain kernels whose oscillator is a
phase accumulator.  The translation unit is compiled to assembly here and every instantiation is checked: present by name, the Q15 products
are v_dot2, the sine comes out of LDS one dword at a time, no scratch, at most 128 vector registers, no private segment and no spills, and no
static LDS -- the whole of it is the launch's dynamic size, pcn_lds_bytes / f32pcn_lds_bytes, which a host program evaluates for the
reference shape.  Also the host side of the new calls: declared in include/msdr.h, exported by libmsdr.so, the flavour bit an enumerator and
mirrored in the Python binding.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minimal-sdr_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
# the product's flags (minimal-sdr_amd/Makefile: HIPFLAGS)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fwrapv", "-fno-slp-vectorize"]
Q15 = tuple("chain_q15pcn_kernelILi%dEE" % cpw for cpw in (1, 2, 4))
F32 = tuple("chain_f32pcn_kernelILi%dEE" % cpw for cpw in (1, 2, 4))
INSTANCES = Q15 + F32


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = os.path.join(str(tmp_path_factory.mktemp("ncopc")), "msdr_chain_ncopc.s")
    subprocess.run([HIPCC] + FLAGS + ["-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "msdr_chain_ncopc.hip")], check=True,
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


def test_every_instantiation_is_present_with_its_products_and_without_scratch_traffic(asm):
    for needle in INSTANCES:
        name, ins = _body(asm, needle)
        if needle in Q15:
            assert sum(1 for i in ins if i.startswith("v_dot2")) >= 64, name          # one step = 8 taps x 8 outputs per filter
        assert not [i for i in ins if "scratch_" in i], name


def test_the_sine_is_read_from_lds_one_dword_at_a_time(asm):
    """The table is written to LDS behind the channels' areas and the mix gathers from it entry by entry (ds_read_b32); the FIR phase reads
    whole 16-byte slots."""
    for needle in INSTANCES:
        name, ins = _body(asm, needle)
        reads = [i.split()[0] for i in ins if i.startswith("ds_read") or i.startswith("ds_load")]
        assert any(r.endswith("_b128") for r in reads), name
        assert any(r.endswith("_b32") for r in reads), (name, sorted(set(reads)))
        assert sum(1 for i in ins if i.startswith("ds_write") or i.startswith("ds_store")) >= 3, (name, "tap rows, sine table, window")


def test_every_instantiation_keeps_to_128_vector_registers_zero_scratch_and_dynamic_lds(asm):
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
        assert int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1)) == 0, name      # all of the LDS is the launch's pcn_lds_bytes
    assert seen == len(INSTANCES), seen


def test_lds_geometry_for_the_reference_shape(tmp_path):
    """pcn_lds_bytes / f32pcn_lds_bytes (the kernels' header, host side) for the reference's 102 taps at 128 samples per call: chain_q15pc_kernel's /
    chain_f32pc_kernel's bytes for 4 waves of 4 channels -- no row per channel -- plus ONE 4 096-byte sine table per workgroup"""
    src = os.path.join(str(tmp_path), "geo.hip")
    with open(src, "w") as f:
        f.write('#include <cstdio>\n#include "msdr_chain_ncopc.hiph"\nusing namespace msdr;\n'
                'int main() { printf("%zu %zu %zu %zu %d %d\\n", pcn_lds_bytes(104, 4, 4), pc_lds_bytes(104, 4, false, 4), f32pcn_lds_bytes(104, 4, 4),\n'
                '                    f32pc_lds_bytes(104, 4, false, false, 4), pcn_max_taps(), f32pcn_max_taps()); return 0; }\n')
    exe = os.path.join(str(tmp_path), "geo")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", "-I" + CSRC, "-o", exe, src], check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    q, q0, f, f0, qmax, fmax = (int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split())
    assert q == q0 + 4096 == 16 * 2 * (4 * (128 + 104) + 2 * 104) + 4096
    assert f == f0 + 4096 == 16 * 4 * (2 * 256 + 2 * 128) + 4096
    assert q <= 65536 and f <= 65536
    assert qmax == 4776 and fmax == 3584                                   # 12 np + 8 192 <= 65 536; 16 np' + 8 192 <= 65 536, np' a multiple of 64


def test_the_new_calls_are_declared_exported_and_mirrored(tmp_path):
    with open(os.path.join(ROOT, "include", "msdr.h")) as f:
        h = f.read()
    for decl in (r"^uint32_t msdr_nco_step\(double f_hz, double fs_hz\);", r"^void msdr_nco_table\(int16_t table\[1025\]\);",
                 r"^void msdr_nco_q15\(const uint32_t \*phase, size_t count, int16_t \*sin_out, int16_t \*cos_out\);",
                 r"^int msdr_chain_set_nco_channels\(", r"^int msdr_chain_get_nco\("):
        assert re.search(decl, h, re.M), decl
    assert re.search(r"^enum \{ MSDR_FLAVOUR_NCO_PC = 0x80000u \};", h, re.M)           # an enumerator: tests/test_abi.py counts the macros
    lib = os.path.join(ROOT, "minimal-sdr_amd", "lib", "libmsdr.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    for sym in ("msdr_nco_step", "msdr_nco_table", "msdr_nco_q15", "msdr_chain_set_nco_channels", "msdr_chain_get_nco"):
        assert re.search(r" T %s$" % sym, out, re.M), sym
    src = os.path.join(str(tmp_path), "size.c")
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include "msdr.h"\nint main(void) { printf("%zu %u\\n", sizeof(msdr_chain_config), (unsigned)MSDR_FLAVOUR_NCO_PC); return 0; }\n')
    exe = os.path.join(str(tmp_path), "size")
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), "-o", exe, src])
    size, bit = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
    import msdr
    assert int(size) == C.sizeof(msdr.ChainConfig) == 264          # the struct as every earlier build laid it out (LP64)
    assert int(bit) == msdr.FLAVOUR_NCO_PC == 0x80000
    assert not msdr.FLAVOUR_NCO_PC & (msdr.FLAVOUR_TAPS_PC | msdr.FLAVOUR_CASCADE_PC | msdr.FLAVOUR_OSC_PC | msdr.FLAVOUR_SHARED_IF | 0x7FFF)
