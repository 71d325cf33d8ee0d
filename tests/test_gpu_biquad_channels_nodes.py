"""tests/cpp/test_biquad_channels.cpp: the sketch's output path queue_dac -> biquad1_dac -> biquad2_dac over the AudioStream runtime with
biquad2_dac.channel(rx).setNotch(...) for every receiver -- half of them queued before AudioGPU.begin, a range retuned while the graph
runs -- built here with g++ against libmsdr.so into a temporary directory and compared with the blocks the oracle computes per receiver."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "minimal-sdr_amd", "lib")


def build(tmp):
    exe = os.path.join(str(tmp), "test_biquad_channels")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_biquad_channels.cpp"),
                           os.path.join(ROOT, "minimal-sdr_amd", "host", "AudioStream.cpp"),
                           "-L" + LIBDIR, "-lmsdr", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_program_builds_and_its_setters_queue_without_a_gpu(tmp_path):
    exe = build(tmp_path)
    out = subprocess.run([exe, "--no-gpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "no-gpu path: OK" in out.stdout


@pytest.mark.gpu
def test_every_receiver_its_own_notch_through_the_node_graph(tmp_path, orc):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
    import msdr
    import orclib
    exe = build(tmp_path)
    rng = np.random.default_rng(8)
    channels, blocks, B = 70, 6, 128
    corr = orclib.AUDIO_SAMPLE_RATE_EXACT / 24000.0
    hz = ((3000.0 + 0.37 * np.arange(channels)) * corr).astype(np.float32)
    first, count, at = 20, 33, 3
    hz2 = ((2600.0 + 1.1 * np.arange(count)) * corr).astype(np.float32)
    lp = np.array([6000 * 0.9 * corr, 0.54], np.float32)
    x = rng.integers(-32768, 32768, (blocks, channels, B)).astype(np.int16)
    x[1, :, 40:60] = 32767
    x[4, :, 10:20] = -32768

    def design(kind, f, q):
        return msdr.biquad_design(kind, np.float32(f), float(np.float32(q)))

    want = np.empty_like(x)
    for c in range(channels):
        n1 = orc.biquad_teensy_new([design(msdr.BQ_LOWPASS, lp[0], lp[1])])
        n2 = orc.biquad_teensy_new([design(msdr.BQ_NOTCH, hz[0], 15.0)])      # the bank-wide default first, then this receiver's own
        orc.lib.orc_biquad_teensy_set_coefficients(C.byref(n2), C.c_uint32(0), orclib._ptr(design(msdr.BQ_NOTCH, hz[c], 15.0)))
        for k in range(blocks):
            if k == at and first <= c < first + count:
                orc.lib.orc_biquad_teensy_set_coefficients(C.byref(n2), C.c_uint32(0), orclib._ptr(design(msdr.BQ_NOTCH, hz2[c - first], 15.0)))
            want[k, c] = orc.biquad_teensy_update(n2, orc.biquad_teensy_update(n1, x[k, c]))
    hz.tofile(os.path.join(str(tmp_path), "notch_hz.bin"))
    np.concatenate([np.array([at, first, count], np.float32), hz2]).tofile(os.path.join(str(tmp_path), "retune.bin"))
    lp.tofile(os.path.join(str(tmp_path), "lowpass.bin"))
    x.tofile(os.path.join(str(tmp_path), "x.bin"))
    want.tofile(os.path.join(str(tmp_path), "want.bin"))
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("OK"), out.stdout
