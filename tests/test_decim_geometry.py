"""The launch geometry of the decimating per-receiver chain kernels (minimal-sdr_amd/csrc/msdr_decpc_geometry.h), without a GPU and without
HIP: a small program compiled with g++ prints dec_geometry, dec_max_taps and dec_max_decimation over a grid of shapes, and the lines are
compared with a Python statement of the documented rule (everything counts OUTPUTS, nout = n / D):

  channels per wave   4 / 2 / 1 for calls of up to 128 / up to 256 / more outputs; outputs per lane 8; tile = OPL * 64 / CPW
  fit                 OPL halved down to 2, then the waves from 4 down to 1, then the channels per wave, until 64 KB of LDS hold; refused
                      where one wave with one channel and two outputs per lane does not fit
  time segments       pc_geometry's rule over the tiles of outputs
  LDS                 Q15: copies x 2 streams x (tile D + np) shorts + 2 np shorts per channel, copies = 2 for odd D; F32: 2 x (tile D + np)
                      + 2 np floats; + 4 096 bytes of sine table per workgroup

and with the limits that include/msdr.h documents for msdr_chain_set_decimation."""
import itertools
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minimal-sdr_amd", "csrc")
CAP = 64 * 1024
DS = list(range(1, 65))
NPS = [8, 104, 504, 4096]
NOUTS = [32, 128, 129, 256, 768, 16384]
CHANNELS = [1, 11, 4096]
CUS = [1, 256]
SEGS = [0, 1, 3]

PROBE = r"""
#include <cstdio>
#include "msdr_decpc_geometry.h"
int main()
{
    using namespace msdr;
    const long long nouts[] = {32, 128, 129, 256, 768, 16384};
    const int nps[] = {8, 104, 504, 4096}, chs[] = {1, 11, 4096}, cus[] = {1, 256}, segs[] = {0, 1, 3};
    for (int f = 0; f < 2; f++) for (int D = 1; D <= 64; D++) for (int np : nps) for (long long nout : nouts) for (int ch : chs) for (int cu : cus) for (int ts : segs) {
        DecGeometry g;
        auto bytes = [&](int cpw, int nw, int opl) { return dec_lds_bytes(f == 1, np, D, cpw, nw, opl); };
        if (!dec_geometry(nout, ch, cu, ts, kPcLdsCap, bytes, &g)) { printf("g %d %d %d %lld %d %d %d refused\n", f, D, np, nout, ch, cu, ts); continue; }
        printf("g %d %d %d %lld %d %d %d %u %u %zu %d %d %d %lld %d %d\n", f, D, np, nout, ch, cu, ts, g.launch.grid, g.launch.block, g.launch.lds_bytes, g.launch.cpw,
               g.launch.nseg, g.launch.tile, g.seg_len, g.nw, g.opl);
    }
    for (int f = 0; f < 2; f++) for (int D = 1; D <= 130; D++) printf("t %d %d %d %d\n", f, D, dec_max_taps(f == 1, D), dec_fits(f == 1, f ? 4 : 8, D) ? 1 : 0);
    printf("m %d %d\n", dec_max_decimation(false), dec_max_decimation(true));
    return 0;
}
"""


# ---- the rule, restated ---------------------------------------------------------------------------------------------------------------------
def lds_bytes(f32, np_, D, cpw, nw, opl):
    tile = opl * (64 // cpw)
    if f32:
        per = 4 * (2 * (tile * D + np_) + 2 * np_)
    else:
        per = 2 * (2 * (2 if D & 1 else 1) * (tile * D + np_) + 2 * np_)
    return per * cpw * nw + 4096


def fit(f32, np_, D, nout):
    cpw, nw, opl = (4 if nout <= 128 else 2 if nout <= 256 else 1), 4, 8
    size = lambda: lds_bytes(f32, np_, D, cpw, nw, opl)          # noqa: E731
    while size() > CAP and opl > 2:
        opl //= 2
    while size() > CAP and nw > 1:
        nw //= 2
    while size() > CAP and cpw > 1:
        cpw //= 2
    return (cpw, nw, opl, size()) if size() <= CAP else None


def geometry(f32, D, np_, nout, ch, cus, ts):
    f = fit(f32, np_, D, nout)
    if f is None:
        return None
    cpw, nw, opl, lds = f
    tile = opl * (64 // cpw)
    groups, tiles = -(-ch // cpw), -(-nout // tile)
    nseg = max(1, min(-(-32 * cus // groups), tiles // 4))
    if ts == 1:
        nseg = 1
    elif ts > 1:
        nseg = max(1, min(ts, tiles))
    seg_tiles = -(-tiles // nseg)
    nseg = -(-tiles // seg_tiles)
    return (-(-groups * nseg // nw), 64 * nw, lds, cpw, nseg, tile, seg_tiles * tile, nw, opl)


def max_taps(f32, D):
    """include/msdr.h: Q15, even D: 512 D + 8 np <= 61 440; Q15, odd D: 1024 D + 12 np <= 61 440; F32: 1024 D + 16 np <= 61 440"""
    if f32:
        return max(0, (61440 - 1024 * D) // 16 // 4 * 4)
    return max(0, ((61440 - 1024 * D) // 12 if D & 1 else (61440 - 512 * D) // 8) // 8 * 8)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    d = tmp_path_factory.mktemp("decim_geometry")
    src, exe = str(d / "probe.cpp"), str(d / "probe")
    with open(src, "w") as f:
        f.write(PROBE)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, "-o", exe, src])
    return [ln.split() for ln in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()]


def test_launch_geometry_follows_the_documented_rule(probe):
    lines = [ln[1:] for ln in probe if ln[0] == "g"]
    assert len(lines) == 2 * len(DS) * len(NPS) * len(NOUTS) * len(CHANNELS) * len(CUS) * len(SEGS)
    want = itertools.product(range(2), DS, NPS, NOUTS, CHANNELS, CUS, SEGS)
    refused = launched = split = 0
    seen = set()
    for ln, (f, D, np_, nout, ch, cus, ts) in zip(lines, want):
        assert [int(v) for v in ln[:7]] == [f, D, np_, nout, ch, cus, ts]
        g = geometry(f, D, np_, nout, ch, cus, ts)
        # it refuses exactly where one wave with one channel (two outputs per lane: a tile of 128) does not fit
        assert (g is None) == (lds_bytes(f, np_, D, 1, 1, 2) > CAP), ln
        if g is None:
            assert ln[7:] == ["refused"], ln
            refused += 1
            continue
        assert tuple(int(v) for v in ln[7:]) == g, (ln, g)
        grid, block, lds, cpw, nseg, tile, seg_len, nw, opl = g
        assert lds <= CAP and block == 64 * nw and tile == opl * (64 // cpw) and opl in (2, 4, 8), ln
        # segments are whole tiles, and the segments [s seg_len, (s + 1) seg_len) cover every output exactly once with no empty segment
        assert seg_len % tile == 0 and nseg * seg_len >= nout > (nseg - 1) * seg_len, ln
        assert grid * nw >= -(-ch // cpw) * nseg > (grid - 1) * nw, ln
        # ... and inside a tile the kernels' lane-to-output mapping (lane g of a channel: outputs r LPC + g, r < opl) does the same
        if (cpw, opl) not in seen:
            seen.add((cpw, opl))
            lpc = 64 // cpw
            assert sorted(r * lpc + gl for r in range(opl) for gl in range(lpc)) == list(range(tile))
        launched += 1
        split += nseg > 1
    assert refused and launched and split
    assert {o for _, o in seen} == {2, 4, 8} and {c for c, _ in seen} == {1, 2, 4}          # (the grid reaches every branch of the fit)
    # the shapes of tests/test_gpu_decim_per_channel.py, 102 taps: (cpw, tile) by nout and D
    assert [geometry(0, 2, 104, n, 11, 256, 0)[3:6:2] for n in (32, 128, 256, 768)] == [(4, 128), (4, 128), (2, 256), (1, 512)]
    assert [geometry(0, 32, 104, n, 11, 256, 0)[3:6:2] for n in (32, 128, 256, 768)] == [(4, 32), (4, 32), (2, 64), (1, 128)]
    # the census (tests/decim_census_cases.py): its three call lengths at an entry whose CPW the fit lowers -- D = 59 beside 48 (Q15) / 36 (fp32)
    # taps leaves room for one wave with one channel and two outputs per lane, whatever n / D chose: (cpw, tile), and the block and the LDS
    assert [geometry(0, 59, 48, n, 2, 256, 0)[3:6:2] for n in (30, 130, 258)] == [(1, 128)] * 3
    assert [geometry(1, 59, 36, n, 2, 256, 0)[3:6:2] for n in (30, 130, 258)] == [(1, 128)] * 3
    assert [geometry(0, 59, 48, n, 2, 256, 0)[:3] for n in (30, 130, 258)] == [(2, 64, 65088)] * 3


def test_the_setters_limits_are_what_the_rule_yields(probe):
    hdr = open(os.path.join(ROOT, "include", "msdr.h")).read()
    m = re.search(r"enum \{ MSDR_MAX_DECIMATION_Q15 = (\d+), MSDR_MAX_DECIMATION_F32 = (\d+) \};", hdr)
    assert m, "include/msdr.h does not declare the maxima"
    (mq, mf), = [[int(v) for v in ln[1:]] for ln in probe if ln[0] == "m"]
    assert (int(m.group(1)), int(m.group(2))) == (mq, mf) == (60, 59)
    assert "1 .. MSDR_MAX_DECIMATION_Q15 (60) / MSDR_MAX_DECIMATION_F32 (59)" in hdr
    taps = {(int(f), int(D)): (int(t), int(ok)) for _, f, D, t, ok in (ln for ln in probe if ln[0] == "t")}
    for f in range(2):
        for D in range(1, 131):
            assert taps[(f, D)][0] == max_taps(f, D), (f, D)
            assert taps[(f, D)][1] == (max_taps(f, D) >= (4 if f else 8)), (f, D)
        # the maximum: every factor up to it holds the shortest filter, the next one does not
        top = (mq, mf)[f]
        assert all(taps[(f, D)][1] for D in range(1, top + 1)) and not taps[(f, top + 1)][1]
    # the header's figures: "At 102 taps every factor up to 58 is accepted; at D = 8 filters of up to 7 168 (Q15) / 3 328 (F32) taps, at D = 32
    # up to 5 632 / 1 792"
    assert "every factor up to 58" in hdr and "7 168" in hdr and "3 328" in hdr and "5 632 / 1 792" in hdr
    for f in range(2):
        assert all(max_taps(f, D) >= 104 for D in range(1, 59)) and max_taps(f, 59) < 104
    assert (max_taps(0, 8), max_taps(1, 8), max_taps(0, 32), max_taps(1, 32)) == (7168, 3328, 5632, 1792)
    for D in (2, 3, 4, 5, 8, 16, 32):          # the factors the interface must accept at 102 taps
        assert max_taps(0, D) >= 104 and max_taps(1, D) >= 104
