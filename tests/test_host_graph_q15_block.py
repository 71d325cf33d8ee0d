"""tests/cpp/test_graph_q15_block.cpp: queue -> AudioSDRDemodulator (MSDR_ARITH_Q15, per-receiver bandwidths and oscillator tables, the chain's
two biquad nodes) -> AudioFilterBiquad -> record queue over the AudioStream runtime -- built here with g++ against libmsdr.so into a temporary
directory.  3 receivers, 8 update_all() ticks; receiver 1 is retuned before tick 4 through setBandwidthChannel / setOscChannel /
setNodeNotchChannel / channel(rx).setNotch.  The program runs once with setBlockKernelQ15 off and once with it on (chain_q15pcb_kernel on every
tick whose history holds no sample of an earlier oscillator table); both captures are the oracle's audio bit for bit, hence each other's."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "minimal-sdr_amd", "lib")
# the program's constants, restated
RETUNE_RX, RETUNE_BLOCK = 1, 4
NEW_BANDWIDTH, LOWPASS, NOTCH, NEW_CHAIN_NOTCH, DAC_NOTCH, NEW_DAC_NOTCH = 1500.0, 5400.0, 3000.0, 2900.0, 3300.0, 3100.0


def build(tmp):
    exe = os.path.join(str(tmp), "test_graph_q15_block")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_graph_q15_block.cpp"),
                           os.path.join(ROOT, "minimal-sdr_amd", "host", "AudioStream.cpp"),
                           "-L" + LIBDIR, "-lmsdr", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_program_builds_and_refuses_bad_arguments_without_a_gpu(tmp_path):
    out = subprocess.run([build(tmp_path), "--no-gpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "no-gpu path: OK" in out.stdout


@pytest.mark.gpu
def test_q15_receivers_one_launch_per_tick_through_the_node_graph(tmp_path, orc):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import orclib
    from gpuhelp import msdr
    exe = build(tmp_path)
    channels, blocks, B, nt = 3, 8, 128, 102
    corr = np.float32(orclib.AUDIO_SAMPLE_RATE_EXACT / 24000.0)          # (the program multiplies in float)

    def taps_of(bw):
        return msdr.calc_fir_coeffs(nt, float(bw), 70.0, 0, 0.0, 24000.0)[:nt].copy()

    def design(kind, f, q):
        return msdr.biquad_design(kind, np.float32(f) * corr, q)

    k = (5 + 7 * np.arange(channels + 1)) % B
    a = 2 * np.pi * k[:, None] * np.arange(B)[None, :] / B + 0.4 * np.arange(channels + 1)[:, None]
    oi, oq = np.round(32767 * np.sin(a)).astype(np.int16), np.round(32767 * np.cos(a)).astype(np.int16)          # the last row pair: the new tables
    x = np.random.default_rng(23).integers(-20000, 20001, (blocks, channels, B)).astype(np.int16)
    for name, arr in (("taps", taps_of(2400.0)), ("osc_i", oi), ("osc_q", oq), ("x", x)):
        np.ascontiguousarray(arr).tofile(os.path.join(str(tmp_path), name + ".bin"))

    want = np.empty_like(x)
    for c in range(channels):
        st = {}
        chain_nodes = [orc.biquad_teensy_new([design(msdr.BQ_LOWPASS, LOWPASS, 0.54)]), orc.biquad_teensy_new([design(msdr.BQ_NOTCH, NOTCH, 15.0)])]
        dac = orc.biquad_teensy_new([design(msdr.BQ_NOTCH, DAC_NOTCH, 15.0)])
        taps, row = taps_of(2000.0 + 400.0 * c), c
        for b in range(blocks):
            if b == RETUNE_BLOCK and c == RETUNE_RX:
                taps, row = taps_of(NEW_BANDWIDTH), channels
                for nd, f in ((chain_nodes[1], NEW_CHAIN_NOTCH), (dac, NEW_DAC_NOTCH)):
                    coef = np.ascontiguousarray(design(msdr.BQ_NOTCH, f, 15.0), np.int32)
                    orc.lib.orc_biquad_teensy_set_coefficients(orclib.C.byref(nd), orclib.C.c_uint32(0), orclib._ptr(coef))
            w = orc.chain_q15(x[b, c], orclib.AM, taps, taps, mixer=1, osc_i=oi[row], osc_q=oq[row], state=st)
            for nd in chain_nodes + [dac]:
                w = orc.biquad_teensy_update(nd, w)
            want[b, c] = w

    got = {}
    for switch in ("off", "on"):
        out = subprocess.run([exe, str(tmp_path), switch], capture_output=True, text=True, timeout=300)
        print(out.stdout)
        assert out.returncode == 0, out.stdout + out.stderr
        assert out.stdout.startswith("OK"), out.stdout
        got[switch] = np.fromfile(os.path.join(str(tmp_path), "got_%s.bin" % switch), np.int16).reshape(blocks, channels, B)
    assert "6 fused ticks" in out.stdout, out.stdout
    assert np.array_equal(got["on"], got["off"])
    for b in range(blocks):
        for c in range(channels):
            assert np.array_equal(got["on"][b, c], want[b, c]), (b, c)
    assert np.abs(want.astype(np.int32)).max() > 100
