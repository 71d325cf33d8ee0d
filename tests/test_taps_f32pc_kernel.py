"""chain_f32pc_kernel (csrc/msdr_chain_f32pc.hiph), without a GPU: the translation unit compiles for gfx950 with the product's flags, every
instantiation is there, its products are fp32 FMAs on the vector ALU, it reads LDS 16 bytes at a time, keeps no scratch and stays inside 128
vector registers; the new entry points are declared and exported; the Python setters refuse malformed arrays before any library call."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minimal-sdr_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
NAMES = ["chain_f32pc_kernelILi%dELb%dELb%dEEE" % (cpw, fir, fs4) for cpw in (1, 2, 4) for fir, fs4 in ((1, 0), (0, 1), (0, 0))]


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc not found at %s" % HIPCC)
    mk = open(os.path.join(ROOT, "minimal-sdr_amd", "Makefile")).read()
    cxx = re.search(r"^CXXFLAGS := (.*)$", mk, re.M).group(1).split()
    hip = [f for f in re.search(r"^HIPFLAGS := (.*)$", mk, re.M).group(1).split() if not f.startswith("$(") and not f.startswith("--offload-arch")]
    out = str(tmp_path_factory.mktemp("f32pc") / "f32pc.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950"] + cxx + hip + ["-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "msdr_chain_f32pc.hip")])
    return open(out).read()


def bodies(asm):
    out = {}
    for n in NAMES:
        m = re.search(r"^(_ZN4msdr18%sv\w*):[^\n]*\n(.*?)\n\s*s_endpgm" % re.escape(n), asm, re.M | re.S)
        assert m, "instantiation %s missing" % n
        out[n] = (m.group(1), m.group(2))
    return out


def test_makefile_and_launcher_declaration():
    mk = open(os.path.join(ROOT, "minimal-sdr_amd", "Makefile")).read()
    assert "$(OUT)/msdr_chain_f32pc.o" in re.search(r"^KOBJ := (.*)$", mk, re.M).group(1)
    assert "launch_chain_f32pc" in open(os.path.join(CSRC, "msdr_block.h")).read()
    assert "struct PcfParams" in open(os.path.join(CSRC, "msdr_shared.h")).read()


def test_every_instantiation_is_fp32_fma_with_wide_lds_reads_and_no_scratch(asm):
    for n, (sym, body) in bodies(asm).items():
        fma = len(re.findall(r"\bv_fma_f32|\bv_fmac_f32", body)) + 2 * len(re.findall(r"\bv_pk_fma_f32", body))          # (v_fmac_f32: the FMA's accumulating encoding)
        fs4_or_fir = "Lb1ELb0" in n or "Lb0ELb1" in n
        step = 32 if fs4_or_fir else 64                      # 4 taps x 8 outputs per stream
        assert fma >= step, (n, fma)
        assert not re.search(r"v_mfma|v_dot2", body), n
        assert len(re.findall(r"\bds_read_b128\b|\bds_load_b128\b", body)) >= 3, n
        assert not re.search(r"\bscratch_", body), n
        blk = [b for b in asm.split("  - .agpr_count:")[1:] if re.search(r"\.name:\s+%s\b" % re.escape(sym), b)]
        assert len(blk) == 1, n
        agpr = int(blk[0].split()[0])
        vgpr = int(re.search(r"\.vgpr_count:\s+(\d+)", blk[0]).group(1))
        print(n, "fma", fma, "vgpr", vgpr, "agpr", agpr)
        assert vgpr + agpr <= 128, (n, vgpr, agpr)
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk[0]).group(1)) == 0 and int(re.search(r"\.sgpr_spill_count:\s+(\d+)", blk[0]).group(1)) == 0, n
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk[0]).group(1)) == 0, n


def test_fs4_flavour_does_half_the_products(asm):
    b = bodies(asm)
    count = lambda n: len(re.findall(r"\bv_fma_f32|\bv_fmac_f32", b[n][1])) + 2 * len(re.findall(r"\bv_pk_fma_f32", b[n][1]))
    for cpw in (1, 2, 4):
        fs4, nco = count("chain_f32pc_kernelILi%dELb0ELb1EEE" % cpw), count("chain_f32pc_kernelILi%dELb0ELb0EEE" % cpw)
        assert fs4 * 2 <= nco + 16, (cpw, fs4, nco)


def test_symbols_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "msdr.h")).read()
    for sym in ("msdr_chain_set_taps_channels_f32", "msdr_fir_f32_set_coeffs_channels"):
        assert re.search(r"^int %s\(" % sym, hdr, re.M), sym
    assert re.search(r"\bMSDR_FLAVOUR_TAPS_PC = 0x8000u\b", hdr)
    assert re.search(r"#define MSDR_MAX_TAPSETS\s+8\b", hdr)
    import msdr
    lib = msdr.load_library()
    assert hasattr(lib, "msdr_chain_set_taps_channels_f32") and hasattr(lib, "msdr_fir_f32_set_coeffs_channels")
    assert msdr.MAX_TAPSETS == 8 and msdr.FLAVOUR_TAPS_PC == 0x8000
    import ctypes as C
    assert C.sizeof(msdr.ChainConfig) == 264


def test_python_setters_refuse_malformed_arrays_before_any_library_call():
    import msdr

    class NoLib:
        def __getattr__(self, name):
            raise AssertionError("library call %s" % name)

    class Ctx:
        lib = NoLib()
    chain = msdr.Chain.__new__(msdr.Chain)
    chain.ctx, chain.h, chain.ntaps, chain.arith = Ctx(), None, 102, msdr.ARITH_F32
    fir = msdr.FirF32.__new__(msdr.FirF32)
    fir.ctx, fir.h, fir.ntaps = Ctx(), None, 102
    good = np.zeros((3, 102), np.float32)
    for bad in (np.zeros(102, np.float32), np.zeros((3, 101), np.float32), np.zeros((2, 3, 102), np.float32)):
        with pytest.raises(ValueError):
            chain.set_taps_channels_f32(0, bad)
        with pytest.raises(ValueError):
            chain.set_taps_channels_f32(0, good, bad)
        with pytest.raises(ValueError):
            fir.set_coeffs_channels(0, bad)
    with pytest.raises(ValueError):
        chain.set_taps_channels_f32(0, good, np.zeros((2, 102), np.float32))
    chain.h = fir.h = None          # (nothing to destroy)
