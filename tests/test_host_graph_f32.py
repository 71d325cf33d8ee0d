"""tests/cpp/test_graph_f32.cpp: queue -> AudioSDRDemodulator (MSDR_ARITH_F32 | MSDR_CHAIN_OUT_I16, per-receiver taps, a per-receiver notch, the
block kernel on) -> record queue over the AudioStream runtime -- built here with g++ against libmsdr.so into a temporary directory.  3
receivers, 4 update_all() ticks; the audio is within 1 LSB of the oracle's fp32 chain converted as arm_float_to_q15 converts (truncation
towards zero of v * 32768, saturated): the tolerance MSDR_CHAIN_OUT_I16 documents."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "minimal-sdr_amd", "lib")


def build(tmp):
    exe = os.path.join(str(tmp), "test_graph_f32")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_graph_f32.cpp"),
                           os.path.join(ROOT, "minimal-sdr_amd", "host", "AudioStream.cpp"),
                           "-L" + LIBDIR, "-lmsdr", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_program_builds_and_refuses_bad_arguments_without_a_gpu(tmp_path):
    out = subprocess.run([build(tmp_path), "--no-gpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "no-gpu path: OK" in out.stdout


@pytest.mark.gpu
def test_fp32_receivers_one_launch_per_tick_through_the_node_graph(tmp_path, orc):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cascade_pc_cases as cc
    import orclib
    from f32pc_cases import FS4, bw_taps
    exe = build(tmp_path)
    channels, blocks, B = 3, 4, 128
    taps = np.stack([bw_taps(bw) for bw in (1800.0, 2400.0, 3300.0)])
    bq = np.stack([cc.notch(f, q) for f, q in cc.CHAIN_NOTCHES])          # [3, 5]
    x = np.random.default_rng(17).integers(-20000, 20001, (blocks, channels, B)).astype(np.int16)
    want = np.empty_like(x)
    for c in range(channels):
        st = {}
        for k in range(blocks):
            w = orc.chain_f32(x[k, c], orclib.AM, taps[c], taps[c], FS4[0], FS4[1], bq[c][None], state=st)
            want[k, c] = np.clip(np.trunc(w.astype(np.float32) * np.float32(32768.0)), -32768, 32767).astype(np.int16)
    for name, a in (("taps", taps), ("bq", bq), ("x", x), ("want", want)):
        np.ascontiguousarray(a).tofile(os.path.join(str(tmp_path), name + ".bin"))
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("OK"), out.stdout
