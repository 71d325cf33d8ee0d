"""The launch geometry of the per-receiver chain kernels (minimal-sdr_amd/csrc/msdr_pc_geometry.h), without a GPU and without HIP: a small
program compiled with g++ prints pc_geometry / pc_fit_lds over a grid of shapes for every kernel family, and the lines are compared with a
Python statement of the documented rule:

  channels per wave   4 / 2 / 1 for calls of up to 128 / up to 256 / more samples; tile = 8 * 64 / CPW
  waves               halved from 4, then the channels per wave halved, until 64 KB of LDS hold; refused where 1 x 1 does not fit
  time segments       clamp(ceil(32 CUs / channel groups), 1, tiles / 4), overridden by time_segments (1: never split, > 1: that many as far
                      as there are tiles), then renormalised: seg_tiles = ceil(tiles / nseg), nseg = ceil(tiles / seg_tiles)

The LDS layouts of the families are restated twice, in the program (C++) and here (Python), from the comments of the kernels' headers; a second
program, compiled with hipcc against the kernels' headers, prints what the sizing functions the launchers pass (pc_lds_bytes, f32pc_lds_bytes,
pco_lds_bytes, f32pco_lds_bytes, f32pcb_lds_bytes, pcn_lds_bytes, f32pcn_lds_bytes) give, and the restatement is held to them.
The GPU half of this file is the census of tests/pc_census_cases.py (tests/test_gpu_pc_census.py, tests/test_gpu_pc_census_f32.py): every
geometry this rule can reach, run on the kernels and held to the oracle."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minimal-sdr_amd", "csrc")
CAP = 64 * 1024
NS = [8, 100, 128, 129, 256, 512, 1003, 16384, 1 << 20]
NPS = [8, 104, 512, 2048, 3840]
CHANNELS = [1, 5, 64, 4096]
CUS = [1, 256]
SEGS = [0, 1, 3]
OSCS = [0, 24, 128, 8192]
FAMILIES = ["q15pc", "q15fir", "f32pc", "f32fs4", "f32fir", "q15pco", "f32pco", "f32pcb"]
# the kernels with a phase-accumulator oscillator: the channel areas of q15pc / f32pc and, ONCE per workgroup, the packed sine table (kPcnTabBytes)
NCO_FAMILIES = {"q15pcn": "q15pc", "f32pcn": "f32pc"}
TAB_BYTES = 4 * 1024

PROBE = r"""
#include <cstdio>
#include "msdr_pc_geometry.h"
static long long up(long long v, long long m) { return (v + m - 1) / m * m; }
// bytes of LDS of a workgroup: family f, np taps per row, osc_len entries, cpw channels per wave, nw waves
static size_t lds(int f, int np, int o, int cpw, int nw)
{
    const long long tile = 8 * (64 / cpw);
    long long per = 0;
    switch (f) {
    case 0: per = 2 * (4 * (tile + np) + 2 * np); break;                                              // q15pc: 4 window copies, 2 tap rows, shorts
    case 1: per = 2 * (2 * (tile + np) + np); break;                                                  // q15fir
    case 2: per = 4 * (2 * up(tile + np, 64) + 2 * up(np, 64)); break;                                // f32pc: 2 windows, 2 rows, whole 256-byte rows
    case 3: per = 4 * (up(tile + np, 64) + 2 * up(np, 64)); break;                                    // f32fs4: one window
    case 4: per = 4 * (up(tile + np, 64) + up(np, 64)); break;                                        // f32fir
    case 5: per = 2 * (4 * (tile + np) + 2 * np) + 4 * up(o, 4); break;                               // q15pco: + one dword per entry
    case 6: per = 4 * (2 * up(tile + np, 64) + 2 * up(np, 64) + up(2 * o, 64)); break;                // f32pco: + one float2 per entry
    default: per = 4 * ((o ? 2 : 1) * up(tile + np, 64) + 2 * up(np, 64) + (o ? up(2 * o, 64) : 0) + tile); break;   // f32pcb: + the output row
    }
    return (size_t)per * cpw * nw;
}
int main()
{
    const long long ns[] = {8, 100, 128, 129, 256, 512, 1003, 16384, 1 << 20};
    const int nps[] = {8, 104, 512, 2048, 3840}, chs[] = {1, 5, 64, 4096}, cus[] = {1, 256}, segs[] = {0, 1, 3}, oscs[] = {0, 24, 128, 8192};
    for (int f = 0; f < 8; f++) for (long long n : ns) for (int np : nps) for (int o : oscs) {
        auto bytes = [&](int cpw, int nw) { return lds(f, np, o, cpw, nw); };
        if (f == 7) {          // the block kernel: the fitting step alone
            int cpw = 0, nw = 0;
            const bool ok = msdr::pc_fit_lds(n, msdr::kPcLdsCap, bytes, &cpw, &nw);
            printf("%d %lld %d %d fit %d %d %d %zu\n", f, n, np, o, ok ? 1 : 0, cpw, nw, ok ? bytes(cpw, nw) : (size_t)0);
            continue;
        }
        for (int ch : chs) for (int cu : cus) for (int ts : segs) {
            msdr::PcGeometry g;
            if (!msdr::pc_geometry(n, ch, cu, ts, 8, msdr::kPcLdsCap, bytes, &g)) { printf("%d %lld %d %d %d %d %d refused\n", f, n, np, o, ch, cu, ts); continue; }
            printf("%d %lld %d %d %d %d %d %u %u %zu %d %d %d %lld %d\n", f, n, np, o, ch, cu, ts, g.launch.grid, g.launch.block, g.launch.lds_bytes, g.launch.cpw,
                   g.launch.nseg, g.launch.tile, g.seg_len, g.nw);
        }
    }
    return 0;
}
"""

# the kernels' own sizing functions, family by family in the order of FAMILIES (host code of a HIP translation unit: the headers need HIP)
SIZES = r"""
#include <cstdio>
#include "msdr_chain_f32pcb.hiph"
#include "msdr_chain_ncopc.hiph"
int main()
{
    using namespace msdr;
    const int nps[] = {8, 104, 512, 2048, 3840}, oscs[] = {0, 24, 128, 8192}, cpws[] = {1, 2, 4}, nws[] = {1, 2, 4};
    printf("%zu\n", kPcnTabBytes);
    for (int np : nps) for (int o : oscs) for (int c : cpws) for (int w : nws)
        printf("%d %d %d %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", np, o, c, w, pc_lds_bytes(np, c, false, w), pc_lds_bytes(np, c, true, w), f32pc_lds_bytes(np, c, false, false, w),
               f32pc_lds_bytes(np, c, false, true, w), f32pc_lds_bytes(np, c, true, false, w), pco_lds_bytes(np, o, c, w), f32pco_lds_bytes(np, o, c, w), f32pcb_lds_bytes(np, o, c, w),
               pcn_lds_bytes(np, c, w), f32pcn_lds_bytes(np, c, w));
    return 0;
}
"""


# ---- the rule, restated ---------------------------------------------------------------------------------------------------------------------
def up(v, m):
    return -(-v // m) * m


def chan_bytes(fam, np_, o, cpw):
    tile = 8 * (64 // cpw)
    if fam in ("q15pc", "q15fir", "q15pco"):
        streams, rows = (1, 1) if fam == "q15fir" else (2, 2)
        return 2 * (2 * streams * (tile + np_) + rows * np_) + (4 * up(o, 4) if fam == "q15pco" else 0)
    streams = 2 if fam in ("f32pc", "f32pco") or (fam == "f32pcb" and o) else 1
    rows = 1 if fam == "f32fir" else 2
    floats = streams * up(tile + np_, 64) + rows * up(np_, 64)
    if fam == "f32pco" or (fam == "f32pcb" and o):
        floats += up(2 * o, 64)
    if fam == "f32pcb":
        floats += tile
    return 4 * floats


def lds_bytes(fam, np_, o, cpw, nw):
    """the workgroup's LDS: cpw x nw channel areas, and behind them what a family keeps once per workgroup"""
    if fam in NCO_FAMILIES:
        return chan_bytes(NCO_FAMILIES[fam], np_, 0, cpw) * cpw * nw + TAB_BYTES
    return chan_bytes(fam, np_, o, cpw) * cpw * nw


def fit(fam, n, np_, o):
    cpw, nw = (4 if n <= 128 else 2 if n <= 256 else 1), 4
    size = lambda: lds_bytes(fam, np_, o, cpw, nw)          # noqa: E731
    while size() > CAP and nw > 1:
        nw //= 2
    while size() > CAP and cpw > 1:
        cpw //= 2
    return (cpw, nw, size()) if size() <= CAP else None


def geometry(fam, n, np_, o, ch, cus, ts):
    f = fit(fam, n, np_, o)
    if f is None:
        return None
    cpw, nw, lds = f
    tile = 8 * (64 // cpw)
    groups, tiles = -(-ch // cpw), -(-n // tile)
    nseg = max(1, min(-(-32 * cus // groups), tiles // 4))
    if ts == 1:
        nseg = 1
    elif ts > 1:
        nseg = max(1, min(ts, tiles))
    seg_tiles = -(-tiles // nseg)
    nseg = -(-tiles // seg_tiles)
    return (-(-groups * nseg // nw), 64 * nw, lds, cpw, nseg, tile, seg_tiles * tile, nw)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("pc_geometry")
    src, exe = str(d / "probe.cpp"), str(d / "probe")
    with open(src, "w") as f:
        f.write(PROBE)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, "-o", exe, src])
    return subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()


def test_launch_geometry_follows_the_documented_rule(probe):
    lines = [ln.split() for ln in probe if ln.split()[4] != "fit"]
    assert len(lines) == 7 * len(NS) * len(NPS) * len(OSCS) * len(CHANNELS) * len(CUS) * len(SEGS)
    want = itertools.product(range(7), NS, NPS, OSCS, CHANNELS, CUS, SEGS)
    refused = launched = split = 0
    for ln, (f, n, np_, o, ch, cus, ts) in zip(lines, want):
        assert [int(v) for v in ln[:7]] == [f, n, np_, o, ch, cus, ts]
        g = geometry(FAMILIES[f], n, np_, o, ch, cus, ts)
        if g is None:
            assert ln[7:] == ["refused"], ln
            refused += 1
            continue
        assert tuple(int(v) for v in ln[7:]) == g, (ln, g)
        grid, block, lds, cpw, nseg, tile, seg_len, nw = g
        assert lds <= CAP and seg_len % tile == 0 and nseg * seg_len >= n > (nseg - 1) * seg_len, ln          # whole tiles, every sample, no empty segment
        assert grid * nw >= -(-ch // cpw) * nseg > (grid - 1) * nw, ln
        launched += 1
        split += nseg > 1
    assert refused and launched and split          # (the grid reaches refusals, launches and calls in time segments)
    # the families without a row ignore osc_len; time_segments = 1 never splits; the rule, not time_segments, splits a long call of few channels
    assert geometry("q15pc", 1 << 20, 104, 0, 5, 256, 0)[4] > 1 and geometry("q15pc", 1 << 20, 104, 0, 5, 256, 1)[4] == 1
    assert geometry("f32pc", 1 << 20, 104, 0, 5, 256, 3)[4] == 3
    # one wave with one channel: 3 840 taps fit the fp32 chain, not beside a row of 8 192 entries
    assert geometry("f32pc", 512, 3840, 0, 1, 1, 0)[3:5] == (1, 1) and geometry("f32pco", 512, 3840, 8192, 1, 1, 0) is None


def test_block_kernel_fit_and_the_figures_of_its_header(probe):
    lines = [ln.split() for ln in probe if ln.split()[4] == "fit"]
    assert len(lines) == len(NS) * len(NPS) * len(OSCS)
    for ln, (n, np_, o) in zip(lines, itertools.product(NS, NPS, OSCS)):
        assert [int(v) for v in ln[:4]] == [7, n, np_, o]
        f = fit("f32pcb", n, np_, o)
        assert tuple(int(v) for v in ln[5:]) == ((1,) + f if f else (0, 0, 0, 0)), (ln, f)
    # msdr_chain_f32pcb.hiph: n = 128, np = 104, osc_len = 128 -- 2 waves and 36 864 bytes; Fs/4 -- 4 waves and 40 960 bytes.  (np = 104 and
    # osc_len = 128 are on the grid, so the program's lines say the same.)
    assert fit("f32pcb", 128, 104, 128) == (4, 2, 36864) and fit("f32pcb", 128, 104, 0) == (4, 4, 40960)
    assert ["7", "128", "104", "128", "fit", "1", "4", "2", "36864"] in lines and ["7", "128", "104", "0", "fit", "1", "4", "4", "40960"] in lines
    assert fit("f32pcb", 128, 3840, 8192) is None


def test_restated_layouts_are_the_kernels_sizing_functions(tmp_path):
    src, exe = str(tmp_path / "sizes.hip"), str(tmp_path / "sizes")
    with open(src, "w") as f:
        f.write(SIZES)
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-fwrapv", "-Wno-unused-value", "-I" + CSRC, "-o", exe, src])
    lines = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()
    assert int(lines[0]) == TAB_BYTES          # kPcnTabBytes
    lines = lines[1:]
    assert len(lines) == len(NPS) * len(OSCS) * 9
    for ln in lines:
        np_, o, cpw, nw, *got = (int(v) for v in ln.split())
        assert got[:8] == [chan_bytes(fam, np_, o, cpw) * cpw * nw for fam in FAMILIES], ln
        assert got == [lds_bytes(fam, np_, o, cpw, nw) for fam in FAMILIES + list(NCO_FAMILIES)], ln
    # the figures of msdr_chain_f32pcb.hiph, from f32pcb_lds_bytes itself
    assert "104 128 4 2 " in "\n".join(lines) and [ln.split()[11] for ln in lines if ln.startswith(("104 128 4 2 ", "104 0 4 4 "))] == ["40960", "36864"]
