"""tests/cpp/test_input_rows.cpp: queue -> AudioSDRDemodulator (NCO mixer) -> record queue over the AudioStream runtime with
demod.setInputRows(n_inputs, rows): 22 receivers, each with oscillator tables of its own, hear 3 rows of the incoming block, and the map
changes while the graph runs -- built here with g++ against libmsdr.so into a temporary directory and compared with the blocks the oracle
computes per receiver on the row it heard at each block."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "minimal-sdr_amd", "lib")


def build(tmp):
    exe = os.path.join(str(tmp), "test_input_rows")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_input_rows.cpp"),
                           os.path.join(ROOT, "minimal-sdr_amd", "host", "AudioStream.cpp"),
                           "-L" + LIBDIR, "-lmsdr", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


@pytest.mark.gpu
def test_one_queue_feeds_the_bank_through_the_node_graph(tmp_path, orc):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
    import msdr
    import orclib
    exe = build(tmp_path)
    rng = np.random.default_rng(17)
    channels, n_inputs, blocks, B, nt, at = 22, 3, 6, 128, 102, 3
    a = 2 * np.pi * (1 + 3 * np.arange(channels) % B)[:, None] * np.arange(B)[None, :] / B + (0.4 * np.arange(channels))[:, None]
    oi, oq = np.round(32767 * np.sin(a)).astype(np.int16), np.round(32767 * np.cos(a)).astype(np.int16)
    map0 = ((7 * np.arange(channels) + 2) % n_inputs).astype(np.uint32)
    map1 = ((5 * np.arange(channels) // 3 + 1) % n_inputs).astype(np.uint32)
    assert set(map0) == set(map1) == set(range(n_inputs)) and (map0 != map1).any()
    am = msdr.calc_fir_coeffs(nt, 2400.0)[:nt].copy()
    x = rng.integers(-20000, 20001, (blocks, n_inputs, B)).astype(np.int16)
    want = np.empty((blocks, channels, B), np.int16)
    for c in range(channels):
        st = {}
        for k in range(blocks):          # the oracle's FIR state is what the receiver heard: an antenna switch at block `at`
            want[k, c] = orc.chain_q15(x[k, (map0 if k < at else map1)[c]], orclib.AM, am, am, mixer=1, osc_i=oi[c], osc_q=oq[c], state=st)
    d = str(tmp_path)
    oi.tofile(os.path.join(d, "osc_i.bin"))
    oq.tofile(os.path.join(d, "osc_q.bin"))
    np.concatenate([np.array([n_inputs, at], np.uint32), map0, map1]).tofile(os.path.join(d, "maps.bin"))
    am.tofile(os.path.join(d, "taps.bin"))
    x.tofile(os.path.join(d, "x.bin"))
    want.tofile(os.path.join(d, "want.bin"))
    out = subprocess.run([exe, d], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("OK"), out.stdout
