"""chain_f32pcb_kernel (minimal-sdr_amd/csrc/msdr_chain_f32pcb.hiph), without a GPU: the translation unit cross-compiles for gfx950 with the
product's flags, every instantiation is there and its code-object metadata shows no scratch (no private segment, no spills); the LDS helper
of the header gives the byte counts of a Python restatement of the layout; the longest filter it accepts at the reference's block fits 64 KB;
the new entry point is declared, exported and bound."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minimal-sdr_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
INSTANCES = ["chain_f32pcb_kernelILi%dELb%dEEE" % (cpw, fs4) for cpw in (1, 2, 4) for fs4 in (0, 1)]
CAP = 64 * 1024


def flags():
    mk = open(os.path.join(ROOT, "minimal-sdr_amd", "Makefile")).read()
    cxx = re.search(r"^CXXFLAGS := (.*)$", mk, re.M).group(1).split()
    hip = [f for f in re.search(r"^HIPFLAGS := (.*)$", mk, re.M).group(1).split() if not f.startswith("$(") and not f.startswith("--offload-arch")]
    return cxx + hip


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("f32pcb") / "f32pcb.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950"] + flags() + ["-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "msdr_chain_f32pcb.hip")])
    return open(out).read()


def test_makefile_builds_the_translation_unit_and_the_launcher_is_declared():
    mk = open(os.path.join(ROOT, "minimal-sdr_amd", "Makefile")).read()
    assert "$(OUT)/msdr_chain_f32pcb.o" in re.search(r"^KOBJ := (.*)$", mk, re.M).group(1)
    blk = open(os.path.join(CSRC, "msdr_block.h")).read()
    assert "launch_chain_f32pcb" in blk and "chain_f32pcb_lds" in blk
    assert "struct PcbParams" in open(os.path.join(CSRC, "msdr_shared.h")).read()


def test_every_instantiation_is_there_without_scratch(asm):
    meta = asm[asm.index("amdhsa.kernels"):]
    seen = set()
    for block in re.split(r"\n\s+- \.agpr_count:", "\n" + meta)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block).group(1)
        hit = [n for n in INSTANCES if n in name]
        if not hit:
            continue
        seen.add(hit[0])
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1)) == 0, name
        assert int(re.search(r"\.vgpr_spill_count:\s+(\d+)", block).group(1)) == 0, name
        assert int(re.search(r"\.sgpr_spill_count:\s+(\d+)", block).group(1)) == 0, name
        assert int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1)) == 0, name          # (dynamic LDS only: the launcher sizes it)
    assert seen == set(INSTANCES), sorted(set(INSTANCES) - seen)


# ---- the layout, restated: floats per channel of a wave, every part rounded up to whole 256-byte rows (64 floats) ----
def up64(v):
    return (v + 63) & ~63


def chan_floats(np_, osc_len, cpw):
    tile = 8 * (64 // cpw)
    streams = 1 if osc_len == 0 else 2                     # osc_len 0: the Fs/4 flavour, one stream and no oscillator row
    return streams * up64(tile + np_) + 2 * up64(np_) + (up64(2 * osc_len) if osc_len else 0) + tile


def geometry(n, np_, osc_len):
    cpw, nw = (4 if n <= 128 else 2 if n <= 256 else 1), 4
    size = lambda: chan_floats(np_, osc_len, cpw) * 4 * cpw * nw          # noqa: E731
    while size() > CAP and nw > 1:
        nw >>= 1
    while size() > CAP and cpw > 1:
        cpw >>= 1
    return (cpw, nw, size()) if size() <= CAP else None


PROBE = r"""
#include <cstdio>
#include "msdr_chain_f32pcb.hiph"
int main()
{
    const int ns[3] = {32, 128, 512}, nps[3] = {8, 104, 256}, oscs[2] = {0, 128};
    for (int n : ns) for (int np : nps) for (int o : oscs) {
        int cpw = 0, nw = 0;
        const bool ok = msdr::f32pcb_geometry(n, np, o, &cpw, &nw);
        printf("%d %d %d %d %d %d %zu\n", n, np, o, ok ? 1 : 0, cpw, nw, ok ? msdr::f32pcb_lds_bytes(np, o, cpw, nw) : (size_t)0);
    }
    for (int o : oscs) {
        int np = 4, cpw = 0, nw = 0;
        while (msdr::f32pcb_geometry(128, np + 4, o, &cpw, &nw)) np += 4;
        msdr::f32pcb_geometry(128, np, o, &cpw, &nw);
        printf("max %d %d %d %d %zu %zu\n", o, np, cpw, nw, msdr::f32pcb_lds_bytes(np, o, cpw, nw), msdr::f32pcb_lds_bytes(np + 4, o, 1, 1));
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("f32pcb_probe")
    src, exe = str(d / "probe.hip"), str(d / "probe")
    with open(src, "w") as f:
        f.write(PROBE)
    subprocess.check_call([HIPCC, "--offload-arch=gfx950", "-O1", "-std=c++17", "-fwrapv", "-Wno-unused-value", "-I" + CSRC, "-o", exe, src])
    return subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()


def test_lds_helper_matches_the_restated_layout(probe):
    rows = [tuple(int(v) for v in ln.split()) for ln in probe if not ln.startswith("max")]
    assert len(rows) == 18
    for n, np_, o, ok, cpw, nw, lds in rows:
        want = geometry(n, np_, o)
        assert ok == 1 and want is not None, (n, np_, o)
        assert (cpw, nw, lds) == want, (n, np_, o, (cpw, nw, lds), want)
        assert lds <= CAP and 8 * (64 // cpw) >= n, (n, np_, o)          # a call is one tile
    # the reference's shape, as the header's comment works it out
    assert geometry(128, 104, 128) == (4, 2, 36864) and geometry(128, 104, 0) == (4, 4, 40960)


def test_longest_accepted_filter_at_128_samples_fits_64k(probe):
    for ln in (l for l in probe if l.startswith("max")):
        _, o, np_, cpw, nw, lds, over = ln.split()
        o, np_, cpw, nw, lds, over = int(o), int(np_), int(cpw), int(nw), int(lds), int(over)
        assert (cpw, nw) == (1, 1) and lds <= CAP < over, ln
        assert geometry(128, np_, o) == (1, 1, lds) and geometry(128, np_ + 4, o) is None, ln
        assert np_ >= 2048, ln                                          # (far beyond every filter of the reference)


def test_entry_point_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "msdr.h")).read()
    assert re.search(r"^int msdr_chain_set_block_kernel\(msdr_chain \*chain, int on\);", hdr, re.M)
    assert len(re.findall(r"#define MSDR_FLAVOUR_[A-Z_]+\s", hdr)) == 13          # existing bits only
    sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
    import msdr
    lib = msdr.load_library()
    assert hasattr(lib, "msdr_chain_set_block_kernel") and hasattr(msdr.Chain, "set_block_kernel")
    assert lib.msdr_chain_set_block_kernel(None, 1) == msdr.STATUS_ARGUMENT_ERROR          # a NULL chain, before any device is looked at
    nodes = open(os.path.join(ROOT, "minimal-sdr_amd", "host", "msdr_nodes.h")).read()
    for name in ("setBlockKernel", "setTapsChannelF32", "setBiquadCoeffsChannel"):
        assert name in nodes, name
