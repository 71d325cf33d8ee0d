"""chain_q15pcb_kernel (minimal-sdr_amd/csrc/msdr_chain_q15pcb.hiph), without a GPU: the translation unit cross-compiles for gfx950 with the
product's flags, every instantiation is there and its code-object metadata shows no scratch (no private segment, no spills) and no static
LDS; the LDS helper of the header gives the byte counts of a Python restatement of the layout; the longest filter it accepts at the
reference's block fits 64 KB and 8 taps more do not; the new entry point is declared, exported, bound and refuses a NULL chain."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minimal-sdr_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
INSTANCES = ["chain_q15pcb_kernelILi%dELb%dEEE" % (cpw, fs4) for cpw in (1, 2, 4) for fs4 in (0, 1)]
CAP = 64 * 1024


def flags():
    mk = open(os.path.join(ROOT, "minimal-sdr_amd", "Makefile")).read()
    cxx = re.search(r"^CXXFLAGS := (.*)$", mk, re.M).group(1).split()
    hip = [f for f in re.search(r"^HIPFLAGS := (.*)$", mk, re.M).group(1).split() if not f.startswith("$(") and not f.startswith("--offload-arch")]
    return cxx + hip


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("q15pcb") / "q15pcb.s")
    subprocess.check_call([HIPCC, "--offload-arch=gfx950"] + flags() + ["-S", "--cuda-device-only", "-o", out, os.path.join(CSRC, "msdr_chain_q15pcb.hip")])
    return open(out).read()


def test_makefile_builds_the_translation_unit_and_the_launcher_is_declared():
    mk = open(os.path.join(ROOT, "minimal-sdr_amd", "Makefile")).read()
    assert "$(OUT)/msdr_chain_q15pcb.o" in re.search(r"^KOBJ := (.*)$", mk, re.M).group(1)
    blk = open(os.path.join(CSRC, "msdr_block.h")).read()
    assert "launch_chain_q15pcb" in blk and "chain_q15pcb_lds" in blk
    assert "struct QpcbParams" in open(os.path.join(CSRC, "msdr_shared.h")).read()


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


# ---- the layout, restated: shorts per channel of a wave ----
def chan_shorts(n, np_, osc_len):
    windows = 4 * (n + np_)                                # I, I moved by one, Q, Q moved by one: n + np samples each
    taps = 2 * np_                                         # I row, Q row
    osc = 2 * ((osc_len + 3) & ~3)                         # one dword per entry, whole 16-byte slots; osc_len 0: the Fs/4 flavour, no row
    return windows + taps + osc + n                        # + the output row


def geometry(n, np_, osc_len):
    cpw, nw = (4 if n <= 128 else 2 if n <= 256 else 1), 4
    size = lambda: chan_shorts(n, np_, osc_len) * 2 * cpw * nw          # noqa: E731
    while size() > CAP and nw > 1:
        nw >>= 1
    while size() > CAP and cpw > 1:
        cpw >>= 1
    return (cpw, nw, size()) if size() <= CAP else None


PROBE = r"""
#include <cstdio>
#include "msdr_chain_q15pcb.hiph"
int main()
{
    const int ns[3] = {32, 128, 512}, nps[3] = {8, 104, 256}, oscs[2] = {0, 128};
    for (int n : ns) for (int np : nps) for (int o : oscs) {
        int cpw = 0, nw = 0;
        const bool ok = msdr::qpcb_geometry(n, np, o, &cpw, &nw);
        printf("%d %d %d %d %d %d %zu\n", n, np, o, ok ? 1 : 0, cpw, nw, ok ? msdr::qpcb_lds_bytes(n, np, o, cpw, nw) : (size_t)0);
    }
    for (int o : oscs) {
        int np = 8, cpw = 0, nw = 0;
        while (msdr::qpcb_geometry(128, np + 8, o, &cpw, &nw)) np += 8;
        msdr::qpcb_geometry(128, np, o, &cpw, &nw);
        printf("max %d %d %d %d %zu %zu\n", o, np, cpw, nw, msdr::qpcb_lds_bytes(128, np, o, cpw, nw), msdr::qpcb_lds_bytes(128, np + 8, o, 1, 1));
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("q15pcb_probe")
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
    assert chan_shorts(128, 104, 128) == 1520 and chan_shorts(128, 104, 0) == 1264
    assert geometry(128, 104, 128) == (4, 4, 48640) and geometry(128, 104, 0) == (4, 4, 40448)


def test_longest_accepted_filter_at_128_samples_fits_64k(probe):
    for ln in (l for l in probe if l.startswith("max")):
        _, o, np_, cpw, nw, lds, over = ln.split()
        o, np_, cpw, nw, lds, over = int(o), int(np_), int(cpw), int(nw), int(lds), int(over)
        assert (cpw, nw) == (1, 1) and lds <= CAP < over, ln
        assert geometry(128, np_, o) == (1, 1, lds) and geometry(128, np_ + 8, o) is None, ln
        assert np_ >= 4096, ln                                          # (every chain: num_taps <= 4096)


def test_entry_point_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "msdr.h")).read()
    assert re.search(r"^int msdr_chain_set_block_kernel_q15\(msdr_chain \*chain, int on\);", hdr, re.M)
    assert len(re.findall(r"#define MSDR_FLAVOUR_[A-Z_]+\s", hdr)) == 13          # existing bits only
    sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
    import msdr
    lib = msdr.load_library()
    assert hasattr(lib, "msdr_chain_set_block_kernel_q15") and hasattr(msdr.Chain, "set_block_kernel_q15")
    assert lib.msdr_chain_set_block_kernel_q15(None, 1) == msdr.STATUS_ARGUMENT_ERROR          # a NULL chain, before any device is looked at
    nodes = open(os.path.join(ROOT, "minimal-sdr_amd", "host", "msdr_nodes.h")).read()
    assert "setBlockKernelQ15" in nodes and "msdr_chain_set_block_kernel_q15" in nodes
