"""The launch geometry of the two-stage decimating chain kernels (minimal-sdr_amd/csrc/msdr_prepc_geometry.h), without a GPU and without HIP:
a small program compiled with g++ prints pre_geometry, pre_fits, pre_max_taps, pre_max_decimation, pre_hist_len and pre_chunks_per_tile over
a grid of shapes, and the lines are compared with the Python statement of the documented rule in tests/prefilter_model.py (everything counts
FINAL outputs, nout = n / (D1 D2)):

  dec_geometry's choice of channels per wave, outputs per lane, waves and time segments (tests/test_decim_geometry.py) over the LDS of
  CPW x nw channel areas -- the one-stage window at factor D2 | tap rows | a stage-1 chunk of 2 x (C D1 + np1) samples, C = LPC max(1, 16 / D1)
  -- + 4 096 bytes of sine table + the prefilter row

and the table of tiles that the GPU tests hold msdr_chain_get_info() to is held to the header here."""
import os
import subprocess

import pytest

import prefilter_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minimal-sdr_amd", "csrc")
D1S = [1, 2, 3, 4, 8, 16, 32, 64]
NP1S = [8, 32, 64, 504]
NP2S = [8, 104, 832]
D2S = [1, 2, 3, 4, 8, 32]
NOUTS = [32, 128, 129, 256, 768, 4096]
CHANNELS = [1, 11, 4096]

PROBE = r"""
#include <cstdio>
#include "msdr_prepc_geometry.h"
int main()
{
    using namespace msdr;
    const int d1s[] = {1, 2, 3, 4, 8, 16, 32, 64}, np1s[] = {8, 32, 64, 504}, np2s[] = {8, 104, 832}, d2s[] = {1, 2, 3, 4, 8, 32}, chs[] = {1, 11, 4096};
    const long long nouts[] = {32, 128, 129, 256, 768, 4096};
    for (int f = 0; f < 2; f++) for (int D1 : d1s) for (int np1 : np1s) for (int np2 : np2s) for (int D2 : d2s) {
        printf("f %d %d %d %d %d %d %d %d %d\n", f, D1, np1, np2, D2, pre_fits(f == 1, np1, D1, np2, D2) ? 1 : 0, pre_max_taps(f == 1, D1, np2, D2),
               pre_max_decimation(f == 1, np1, D1, np2), pre_hist_len(np1, D1, np2));
        for (long long nout : nouts) for (int ch : chs) for (int ts = 0; ts < 4; ts += 3) {
            DecGeometry g;
            if (!pre_geometry(f == 1, nout, ch, 256, ts, np1, D1, np2, D2, &g)) { printf("g %d %d %d %d %d %lld %d %d refused\n", f, D1, np1, np2, D2, nout, ch, ts); continue; }
            printf("g %d %d %d %d %d %lld %d %d %u %u %zu %d %d %d %lld %d %d %d\n", f, D1, np1, np2, D2, nout, ch, ts, g.launch.grid, g.launch.block, g.launch.lds_bytes,
                   g.launch.cpw, g.launch.nseg, g.launch.tile, g.seg_len, g.nw, g.opl, pre_chunks_per_tile(np2, D2, g.launch.tile, D1, g.launch.cpw));
        }
    }
    for (int nt = 0; nt < 20; nt++) printf("p %d %d %d\n", nt, pre_pad_taps(false, nt), pre_pad_taps(true, nt));
    return 0;
}
"""


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("prepc")
    src, exe = d / "probe.cpp", d / "probe"
    src.write_text(PROBE)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", CSRC, "-o", str(exe), str(src)])
    out = subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines()
    return [ln.split() for ln in out]


def test_the_geometry_is_the_documented_rule(lines):
    seen = 0
    for w in lines:
        if w[0] != "g":
            continue
        f, D1, np1, np2, D2, nout, ch, ts = (int(v) for v in w[1:9])
        want = pm.geometry(f == 1, np1, D1, np2, D2, nout, ch, 256, ts)
        if w[9] == "refused":
            assert want is None, w
        else:
            assert want is not None, w
            got = [int(v) for v in w[9:]]
            assert got == [want[k] for k in ("grid", "block", "lds_bytes", "cpw", "nseg", "tile", "seg_len", "nw", "opl", "chunks")], (w, want)
            assert want["lds_bytes"] <= pm.CAP
        seen += 1
    assert seen == 2 * len(D1S) * len(NP1S) * len(NP2S) * len(D2S) * len(NOUTS) * len(CHANNELS) * 2


def test_the_fit_rule_the_limits_and_the_history_formula(lines):
    seen = 0
    for w in lines:
        if w[0] != "f":
            continue
        f, D1, np1, np2, D2, fit, max_taps, max_dec, hist = (int(v) for v in w[1:])
        f32 = f == 1
        assert bool(fit) == pm.fits(f32, np1, D1, np2, D2), w
        assert hist == (np2 - 1) * D1 + np1 - 1, w
        q = 4 if f32 else 8
        # the longest prefilter beside (D1, np2, D2): it fits, one step more does not
        assert max_taps % q == 0 and (max_taps == 0 or pm.fits(f32, max_taps, D1, np2, D2)) and not pm.fits(f32, max_taps + q, D1, np2, D2), w
        # the largest second factor beside (np1, D1, np2): every factor up to it fits, the next does not
        assert all(pm.fits(f32, np1, D1, np2, d) for d in range(1, max_dec + 1)) and not pm.fits(f32, np1, D1, np2, max_dec + 1), w
        if D1 not in pm.FACTORS:
            assert not fit and max_taps == 0 and max_dec == 0, w
        seen += 1
    assert seen == 2 * len(D1S) * len(NP1S) * len(NP2S) * len(D2S)
    # the smallest geometry, as include/msdr.h states it: one wave, one channel, 128 outputs
    assert pm.lds_bytes(False, 32, 8, 104, 4, 1, 1, 2) == 2 * (2 * (128 * 4 + 104) + 2 * 104 + 2 * (64 * 2 * 8 + 32)) + 4096 + 64
    assert pm.lds_bytes(True, 32, 8, 104, 4, 1, 1, 2) == 4 * (2 * (128 * 4 + 104) + 2 * 104 + 2 * (64 * 2 * 8 + 32)) + 4096 + 128
    # the issue's example fits in both arithmetics, and so does a one-stage-equivalent second stage of 832 taps behind it
    assert pm.fits(False, 32, 8, 104, 4) and pm.fits(True, 32, 8, 104, 4) and pm.fits(False, 32, 8, 832, 4)
    assert pm.fits(False, 32, 8, 104, 64) and not pm.fits(True, 32, 8, 104, 64) and not pm.fits(False, 32, 8, 104, 128)


def test_taps_are_padded_to_the_kernels_step(lines):
    for w in lines:
        if w[0] == "p":
            nt, q15, f32 = (int(v) for v in w[1:])
            assert q15 == pm.pad(nt, False) and f32 == pm.pad(nt, True) and q15 % 8 == 0 and f32 % 4 == 0 and 0 <= q15 - nt < 8 and 0 <= f32 - nt < 4


def test_the_table_of_the_gpu_tests_is_the_headers(lines):
    index = {tuple(int(v) for v in w[1:9]): w for w in lines if w[0] == "g" and w[9] != "refused"}
    for arith in ("q15", "f32"):
        f32 = arith == "f32"
        for shape in pm.SHAPES:
            D1, N1, D2 = shape
            np1, np2 = pm.pad(N1, f32), pm.pad(pm.NT2, f32)
            gs = [pm.geometry(f32, np1, D1, np2, D2, nout, pm.CH, 256) for nout in pm.NOUTS]
            assert tuple(g["tile"] for g in gs) == pm.TILES[arith][shape], (arith, shape, [g["tile"] for g in gs])
            if shape in pm.MIN_CHUNKS[arith]:
                assert min(g["chunks"] for g in gs) == pm.MIN_CHUNKS[arith][shape] >= 2, (arith, shape)
            for nout, g in zip(pm.NOUTS, gs):          # where the probe's grid has the shape, the header itself gave this tile
                key = (int(f32), D1, np1, np2, D2, nout, pm.CH, 0)
                if key in index:
                    assert int(index[key][14]) == g["tile"], key
        D1, N1, D2 = pm.SEGMENTED["shape"]
        g = pm.geometry(f32, pm.pad(N1, f32), D1, pm.pad(pm.NT2, f32), D2, pm.SEGMENTED["nout"], pm.CH, 256)
        assert g["nseg"] == pm.SEGMENTED["nseg"][arith] >= 2 and g["tile"] == pm.SEGMENTED["tile"][arith]
    # shapes of the table that the probe's grid covers: (2, 8, 1), (8, 32, 4) and (32, 64, 2) at 11 channels
    assert sum(1 for k in index if k[6] == pm.CH and k[7] == 0 and (k[1], k[2], k[4]) in ((2, 8, 1), (8, 32, 4), (32, 64, 2)) and k[3] == 104) >= 3 * 4
