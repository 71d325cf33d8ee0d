"""May the envelope kernel run Q on accumulator 0's tap fragments?  The table builder asks iqshare_check (minimal-sdr_amd/csrc/msdr_iqshare.h,
pure C++) on the numbers of the two matrices it made; this test compiles that header with g++ into a small program and puts to it the
matrices of the de-interleaved envelope table built here in numpy the way msdr_chain_create builds them (window sample s meets output
column b at delay H + b - s, oscillator phase (rot + s - H) mod 4 of the exact Fs/4 mixer, H = the halo of N + 2 S taps), with the runs
found the way the builder finds them.  Accepted: 24, 64, 256, 512 equal taps behind a two-section cascade at an even rotation (24 taps in a halo of 64 samples).  Refused:
hQ != hI, an odd rotation (the arrays swap), one entry of M[1] off by one ulp of its fp16 lo piece, a table whose runs start at chunk 0
(no cascade: the halo has no spare chunk).  No GPU, no HIP."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minimal-sdr_amd", "csrc")

PROBE = r"""
#include <cstdio>
#include <vector>
#include "msdr_iqshare.h"
// every argument: a file of 13 ints (window samples, j0[2][2], cnt[2][2], sp[2][2]), the scale (double), M0, M1 (doubles)
int main(int argc, char **argv)
{
    for (int a = 1; a < argc; a++) {
        FILE *f = fopen(argv[a], "rb");
        if (!f) return 2;
        int hd[13];
        double scale;
        if (fread(hd, sizeof(int), 13, f) != 13 || fread(&scale, sizeof scale, 1, f) != 1) return 3;
        const size_t n = (size_t)hd[0] * 32;
        std::vector<double> m0(n), m1(n);
        if (fread(m0.data(), sizeof(double), n, f) != n || fread(m1.data(), sizeof(double), n, f) != n) return 4;
        fclose(f);
        int j0[2][2], cnt[2][2], sp[2][2];
        for (int k = 0; k < 4; k++) { j0[k >> 1][k & 1] = hd[1 + k]; cnt[k >> 1][k & 1] = hd[5 + k]; sp[k >> 1][k & 1] = hd[9 + k]; }
        // sp < 0: the merged / dense decision as the table builder makes it -- sparse24_merge on the run's first and last block, where the
        // merged step then sits is of no matter to the check
        for (int o = 0; o < 2; o++)
            for (int src = 0; src < 2; src++) {
                if (sp[o][src] >= 0) continue;
                const double *m = o ? m1.data() : m0.data();
                uint16_t shi[msdr::kSp24FragHalfs], slo[msdr::kSp24FragHalfs];
                uint32_t sidx[64];
                const bool ok = cnt[o][src] >= 2 && msdr::sparse24_merge(m + (size_t)(2 * (16 * j0[o][src]) + src) * 32,
                                                                         m + (size_t)(2 * (16 * (j0[o][src] + cnt[o][src] - 1)) + src) * 32, 64, scale, shi, slo, sidx);
                sp[o][src] = ok ? 2048 * (cnt[0][0] + cnt[0][1] + cnt[1][0] + cnt[1][1]) + 2304 * (2 * o + src) : 0;
            }
        printf("%d\n", msdr::iqshare_check(m0.data(), m1.data(), hd[0], scale, j0, cnt, sp) ? 1 : 0);
    }
    return 0;
}
"""


def lowpass(n, fc=2800.0, fs=24000.0):
    k = np.arange(n) - (n - 1) / 2.0
    h = np.sinc(2 * fc / fs * k) * np.hamming(n)
    return (h / h.sum()).astype(np.float32)


def table(hi, hq, rot=0, sections=2, halo=None):
    """M[0], M[1] ([window sample][32 columns]), the scale, and the header's runs and merged steps as the table builder decides them.
    halo: the chain's halo where it is longer than these taps alone need (None: mf_halo of N + 2 S taps)."""
    n = len(hi)
    halo = halo or (n + 2 * sections - 1 + 31) // 32 * 32
    ki = halo + 32
    oc, os_ = np.array([1.0, 0.0, -1.0, 0.0]), np.array([0.0, 1.0, 0.0, -1.0])
    di, dq = np.asarray(hi, np.float64)[::-1], np.asarray(hq, np.float64)[::-1]       # taps by delay
    m = np.zeros((2, ki, 32))
    for s in range(ki):
        for b in range(32):
            d = halo + b - s
            if 0 <= d < n:
                psi = (rot + s - halo) % 4
                m[0, s, b], m[1, s, b] = di[d] * oc[psi], dq[d] * os_[psi]
    ex = 14 - int(np.frexp(np.abs(m).max())[1])
    j0, cnt, sp = np.zeros((2, 2), np.int32), np.zeros((2, 2), np.int32), np.zeros((2, 2), np.int32)
    for o in range(2):
        for src in range(2):
            chunks = [j for j in range(ki // 32) if np.any(m[o, src + 32 * j:32 * (j + 1):2] != 0.0)]
            if chunks:
                j0[o, src], cnt[o, src] = chunks[0], chunks[-1] - chunks[0] + 1
                assert chunks == list(range(chunks[0], chunks[-1] + 1))
                sp[o, src] = -1                                    # the program decides as the table builder does (sparse24_merge)
    return dict(m=m, scale=float(2.0 ** ex), ki=ki, j0=j0, cnt=cnt, sp=sp)


def off_by_one_lo_ulp(t):
    """One entry of M[1] (odd array, a column b >= 1) whose fp16 lo piece moves by one ulp while its hi piece stays."""
    m, scale = t["m"].copy(), t["scale"]
    for s in range(1, t["ki"], 2):
        for b in range(1, 32):
            v = m[1, s, b] * scale
            if v == 0.0:
                continue
            hi = np.float16(v)
            lo = np.float16(v - float(hi))
            lo2 = np.nextafter(lo, np.float16(np.inf))
            v2 = float(hi) + float(lo2)
            if np.float16(v2) == hi and np.float16(v2 - float(hi)) == lo2 and lo2 != lo:
                m[1, s, b] = v2 / scale
                assert m[1, s, b] * scale == v2
                return dict(t, m=m)
    raise AssertionError("no entry found")


def cases():
    lp = {n: lowpass(n) for n in (24, 64, 256, 512)}
    # (24 + 4 taps alone make a halo of 32 samples, whose chunk 0 holds taps: that table is the refused one below.  With a spare chunk in
    # front -- a halo of 64 -- the same taps pass)
    c = [("equal_%d" % n, table(lp[n], lp[n], halo=64 if n == 24 else None), 1) for n in (24, 64, 256, 512)]
    c.append(("equal_24_own_halo_runs_from_chunk_0", table(lp[24], lp[24]), 0))
    c.append(("rotation_2", table(lp[256], lp[256], rot=2), 1))
    c.append(("asymmetric_equal_pair", table(lp[256] * (1 + 0.5 * np.arange(256) / 256).astype(np.float32), lp[256] * (1 + 0.5 * np.arange(256) / 256).astype(np.float32)), 1))
    c.append(("hq_differs", table(lp[256], lowpass(256, 2200.0)), 0))
    c.append(("odd_rotation", table(lp[256], lp[256], rot=1), 0))
    c.append(("odd_rotation_3", table(lp[256], lp[256], rot=3), 0))
    c.append(("one_lo_ulp", off_by_one_lo_ulp(table(lp[256], lp[256])), 0))
    c.append(("runs_from_chunk_0", table(lp[256], lp[256], sections=0), 0))
    merged_differs = table(lp[256], lp[256])
    merged_differs["sp"] = merged_differs["sp"].copy()
    merged_differs["sp"][0, 0], merged_differs["sp"][1, 1] = 36864, 0           # accumulator 0's run merged, accumulator 1's dense
    c.append(("merged_decision_differs", merged_differs, 0))
    return c


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("iqshare")
    src, exe = tmp / "probe.cpp", tmp / "probe"
    src.write_text(PROBE)
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", CSRC, "-o", str(exe), str(src)], check=True)
    cs = cases()
    files = []
    for name, t, _ in cs:
        f = tmp / (name + ".bin")
        with open(f, "wb") as fh:
            fh.write(struct.pack("13i", t["ki"], *t["j0"].ravel().tolist(), *t["cnt"].ravel().tolist(), *t["sp"].ravel().tolist()))
            fh.write(struct.pack("d", t["scale"]))
            fh.write(np.ascontiguousarray(t["m"][0], np.float64).tobytes())
            fh.write(np.ascontiguousarray(t["m"][1], np.float64).tobytes())
        files.append(str(f))
    out = subprocess.run([str(exe)] + files, check=True, stdout=subprocess.PIPE, text=True).stdout.split()
    assert len(out) == len(cs), out
    return {name: (int(v), want, t) for (name, t, want), v in zip(cs, out)}


@pytest.mark.parametrize("name", [c[0] for c in cases()])
def test_the_check_accepts_the_shifted_block_and_nothing_else(verdicts, name):
    got, want, t = verdicts[name]
    print(name, "runs", t["j0"].tolist(), t["cnt"].tolist(), "verdict", got)
    assert got == want, (name, got, want)


def test_the_accepted_tables_have_the_geometry_the_kernels_are_built_for(verdicts):
    # 256 and 512 taps behind two sections: the runs MwGeomEnv256 / MwGeomEnv512 name (chunks 1 .. N / 32 + 1 of one array each)
    for n in (256, 512):
        t = verdicts["equal_%d" % n][2]
        assert t["j0"].tolist() == [[1, 0], [0, 1]] and t["cnt"].tolist() == [[n // 32 + 1, 0], [0, n // 32 + 1]], (n, t["j0"], t["cnt"])
