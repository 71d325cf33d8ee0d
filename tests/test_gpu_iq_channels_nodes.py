"""tests/cpp/test_iq_channels.cpp: queue -> AudioSDRDemodulator -> record queue over the AudioStream runtime with demod.setIqOut(true) and
demod.readIq after each of 2 ticks through update_all(), 3 receivers with a phase-accumulator oscillator each; built here with g++ against
libmsdr.so into a temporary directory.  The pairs must equal the oracle's (i, q) and the buffer the C ABI reports, and setIqOut(false) must
leave the chain without one."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "minimal-sdr_amd", "lib")


def build(tmp):
    exe = os.path.join(str(tmp), "test_iq_channels")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_iq_channels.cpp"),
                           os.path.join(ROOT, "minimal-sdr_amd", "host", "AudioStream.cpp"),
                           "-L" + LIBDIR, "-lmsdr", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_program_builds_and_refuses_bad_arguments_without_a_gpu(tmp_path):
    exe = build(tmp_path)
    out = subprocess.run([exe, "--no-gpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "no-gpu path: OK" in out.stdout


@pytest.mark.gpu
def test_pairs_of_three_receivers_after_every_tick_through_the_node_graph(tmp_path, orc):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
    import msdr
    import orclib
    exe = build(tmp_path)
    rng = np.random.default_rng(5900)
    channels, blocks, B, nt = 3, 2, 128, 102
    steps = np.array([msdr.nco_step(f) for f in (6000.0, 5992.5, 3000.0)], np.uint64)
    phases = rng.integers(0, 1 << 32, channels, dtype=np.uint64)
    am = msdr.calc_fir_coeffs(nt, 2400.0)[:nt].copy()
    t = np.arange(blocks * B)
    x = np.stack([np.round(20000 * np.cos(2 * np.pi * 6000.0 * t / 24000.0 + c) + rng.normal(0, 50, t.size)).astype(np.int16) for c in range(channels)])
    x = np.ascontiguousarray(x.reshape(channels, blocks, B).transpose(1, 0, 2))
    want = np.empty((blocks, channels, B, 2), np.int16)
    m32 = np.uint64(0xFFFFFFFF)
    for c in range(channels):
        st, phi = {}, phases[c]
        for k in range(blocks):
            ph = (phi + np.arange(B, dtype=np.uint64) * steps[c]) & m32
            phi = (phi + np.uint64(B) * steps[c]) & m32
            s, co = msdr.nco_q15(ph.astype(np.uint32))
            _, i, q = orc.chain_q15(x[k, c], orclib.AM, am, am, mixer=1, osc_i=s, osc_q=co, state=st, want_iq=True)
            want[k, c, :, 0], want[k, c, :, 1] = i, q
    assert np.abs(want[-1, 0].astype(np.int32)).max() > 10 * np.abs(want[-1, 2].astype(np.int32)).max()          # on the carrier / 3 kHz away from it
    np.concatenate([steps, phases]).astype(np.uint32).tofile(os.path.join(str(tmp_path), "nco.bin"))
    am.tofile(os.path.join(str(tmp_path), "taps.bin"))
    x.tofile(os.path.join(str(tmp_path), "x.bin"))
    want.tofile(os.path.join(str(tmp_path), "want.bin"))
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("OK"), out.stdout
