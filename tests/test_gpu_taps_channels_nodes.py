"""tests/cpp/test_taps_channels.cpp: queue -> AudioSDRDemodulator -> record queue over the AudioStream runtime with
demod.setBandwidthChannel(rx, bandwidth) for every receiver and a range of receivers changed while the graph runs -- built here with g++
against libmsdr.so into a temporary directory and compared with the blocks the oracle computes per receiver."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "minimal-sdr_amd", "lib")


def build(tmp):
    exe = os.path.join(str(tmp), "test_taps_channels")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_taps_channels.cpp"),
                           os.path.join(ROOT, "minimal-sdr_amd", "host", "AudioStream.cpp"),
                           "-L" + LIBDIR, "-lmsdr", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_program_builds_and_refuses_bad_arguments_without_a_gpu(tmp_path):
    exe = build(tmp_path)
    out = subprocess.run([exe, "--no-gpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "no-gpu path: OK" in out.stdout


@pytest.mark.gpu
def test_every_receiver_its_own_bandwidth_through_the_node_graph(tmp_path, orc):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
    import msdr
    import orclib
    exe = build(tmp_path)
    rng = np.random.default_rng(12)
    channels, blocks, B, nt = 70, 6, 128, 102
    bw = (125.0 + 25.0 * ((np.arange(channels) * 7) % 196)).astype(np.float32)       # 70 distinct values of the menu's 125 .. 5000 Hz
    first, count, at = 20, 33, 3
    bw2 = (4975.0 - 50.0 * np.arange(count)).astype(np.float32)
    am = msdr.calc_fir_coeffs(nt, 2400.0)[:nt].copy()

    def taps(f):
        return msdr.calc_fir_coeffs(nt, float(f), 70.0, 0, 0.0, 24000.0)[:nt].copy()

    x = rng.integers(-20000, 20001, (blocks, channels, B)).astype(np.int16)
    want = np.empty_like(x)
    for c in range(channels):
        st, t = {}, taps(bw[c])
        for k in range(blocks):
            if k == at and first <= c < first + count:
                t = taps(bw2[c - first])
            want[k, c] = orc.chain_q15(x[k, c], orclib.AM, t, t, state=st)
    bw.tofile(os.path.join(str(tmp_path), "bw_hz.bin"))
    np.concatenate([np.array([at, first, count], np.float32), bw2]).tofile(os.path.join(str(tmp_path), "retune.bin"))
    am.tofile(os.path.join(str(tmp_path), "taps.bin"))
    x.tofile(os.path.join(str(tmp_path), "x.bin"))
    want.tofile(os.path.join(str(tmp_path), "want.bin"))
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("OK"), out.stdout
