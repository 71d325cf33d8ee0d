"""tests/cpp/test_agc.cpp: play queue -> AudioSDRDemodulator with setNco + setInputRows (one antenna row) + setGain / gain / setAgc -> record queue
over the AudioStream runtime, 4 receivers for 6 ticks through update_all(), readAgc behind every tick; built here with g++ against libmsdr.so
into a temporary directory.  Audio and records must equal tests/agc_model.py's."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "minimal-sdr_amd", "lib")


def build(tmp):
    exe = os.path.join(str(tmp), "test_agc")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_agc.cpp"),
                           os.path.join(ROOT, "minimal-sdr_amd", "host", "AudioStream.cpp"),
                           "-L" + LIBDIR, "-lmsdr", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.gpu
def test_four_receivers_with_gain_and_agc_through_the_node_graph(tmp_path, orc):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
    import msdr
    import orclib
    import agc_model as M
    rng = np.random.default_rng(9990)
    channels, blocks, B, nt = 4, 6, 128, 102
    n = blocks * B
    steps = np.array([msdr.nco_step(f) for f in (6000.0, 2310.0, 6000.0, 2310.0)], np.uint64)
    phases = rng.integers(0, 1 << 32, channels, dtype=np.uint64)
    am = msdr.calc_fir_coeffs(nt, 2800.0)[:nt].copy()
    t = np.arange(n)
    x = np.round(20000 * np.cos(2 * np.pi * 6000.0 * t / 24000.0) + 63 * np.cos(2 * np.pi * 2310.0 * t / 24000.0 + 1.0) + rng.normal(0, 1.5, n)).astype(np.int16)
    gains, agc_on = np.array([4.0, 1.0, 0.5, 37.5], np.float32), np.array([1, 1, 0, 0], np.int32)
    m32 = np.uint64(0xFFFFFFFF)
    ph = (phases[:, None] + np.arange(n, dtype=np.uint64)[None, :] * steps[:, None]) & m32
    s, co = msdr.nco_q15(ph.astype(np.uint32))
    si, sq = s.reshape(ph.shape), co.reshape(ph.shape)
    modes = np.full(channels, orclib.AM, np.int32)
    bank = M.BankQ15(orc, x[None, :], None, si, sq, modes, [am] * channels, [am] * channels, rows=[0] * channels)
    for c, rx in enumerate(bank.rx):
        rx.set_gain(gains[c])
        rx.on = int(agc_on[c])
    want, words = np.empty((blocks, channels, B), np.int16), np.empty((blocks, channels, 32), np.int32)
    for k in range(blocks):
        want[k] = bank.call(k * B, (k + 1) * B)[0]
        words[k] = np.stack([rx.words() for rx in bank.rx])
    assert bank.rx[1].val > 1.0 and bank.rx[2].steps == 0 and words[-1, 0, 4] == blocks
    np.concatenate([steps, phases]).astype(np.uint32).tofile(os.path.join(str(tmp_path), "nco.bin"))
    for name, a in (("taps", am), ("gains", gains), ("agc_on", agc_on), ("x", x), ("want", want), ("words", words)):
        np.ascontiguousarray(a).tofile(os.path.join(str(tmp_path), name + ".bin"))
    out = subprocess.run([build(tmp_path), str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("OK"), out.stdout
