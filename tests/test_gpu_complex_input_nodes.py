"""tests/cpp/test_complex_input.cpp: two play queues (I, Q) -> AudioSDRDemodulator with setNco + setComplexInput(true, 0) -> record queue over the
AudioStream runtime, 3 receivers for 2 ticks through update_all(); built here with g++ against libmsdr.so into a temporary directory.  The audio
must equal the composed oracle's (tests/cx_cases.py), and setComplexInput(false, 0) over a cleared history must bring the real-input audio back."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "minimal-sdr_amd", "lib")


def build(tmp):
    exe = os.path.join(str(tmp), "test_complex_input")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_complex_input.cpp"),
                           os.path.join(ROOT, "minimal-sdr_amd", "host", "AudioStream.cpp"),
                           "-L" + LIBDIR, "-lmsdr", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_program_builds_and_refuses_bad_arguments_without_a_gpu(tmp_path):
    exe = build(tmp_path)
    out = subprocess.run([exe, "--no-gpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "no-gpu path: OK" in out.stdout


@pytest.mark.gpu
def test_three_receivers_on_a_complex_stream_through_the_node_graph(tmp_path, orc):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
    import msdr
    import orclib
    from cx_cases import compose_q15
    exe = build(tmp_path)
    rng = np.random.default_rng(7990)
    channels, blocks, B, nt = 3, 2, 128, 102
    n = blocks * B
    steps = np.array([msdr.nco_step(f) for f in (6000.0, 5992.5, 3000.0)], np.uint64)
    phases = rng.integers(0, 1 << 32, channels, dtype=np.uint64)
    am = msdr.calc_fir_coeffs(nt, 2400.0)[:nt].copy()
    t = np.arange(n)
    # a complex exponential at +6 kHz per receiver, and noise: dir 0 brings it down to 0 Hz for receiver 0
    xi = np.stack([np.round(20000 * np.cos(2 * np.pi * 6000.0 * t / 24000.0 + c) + rng.normal(0, 50, n)).astype(np.int16) for c in range(channels)])
    xq = np.stack([np.round(20000 * np.sin(2 * np.pi * 6000.0 * t / 24000.0 + c) + rng.normal(0, 50, n)).astype(np.int16) for c in range(channels)])
    m32 = np.uint64(0xFFFFFFFF)
    want, real = np.empty((channels, n), np.int16), np.empty((channels, n), np.int16)
    for c in range(channels):
        ph = (phases[c] + np.arange(n, dtype=np.uint64) * steps[c]) & m32
        s, co = msdr.nco_q15(ph.astype(np.uint32))
        want[c] = compose_q15(orc, xi[c], xq[c], s, co, 0, orclib.AM, am, am)[0]
        st = {}
        real[c] = np.concatenate([orc.chain_q15(xi[c, o:o + B], orclib.AM, am, am, mixer=1, osc_i=s[o:o + B], osc_q=co[o:o + B], state=st) for o in range(0, n, B)])
    assert np.abs(want[0, B:].astype(np.int32)).min() > 10 * np.abs(want[2, B:].astype(np.int32)).max()          # on the carrier / 3 kHz away from it
    assert not np.array_equal(want, real)

    def blocked(a):
        return np.ascontiguousarray(a.reshape(channels, blocks, B).transpose(1, 0, 2))
    np.concatenate([steps, phases]).astype(np.uint32).tofile(os.path.join(str(tmp_path), "nco.bin"))
    am.tofile(os.path.join(str(tmp_path), "taps.bin"))
    for name, a in (("xi", xi), ("xq", xq), ("want", want), ("real", real)):
        blocked(a).tofile(os.path.join(str(tmp_path), name + ".bin"))
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("OK"), out.stdout
