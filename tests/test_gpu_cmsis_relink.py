"""tests/cpp/test_cmsis_relink.cpp: a C++ program that calls only the CMSIS-DSP names (MSDR_CMSIS_NAMES) -- the FIR section of
demodulation() with arm_copy_q15, freq_conv.cpp's update() as an AudioStream node beside the native AudioEffectFreqConv, and
showSpectrum()'s arm_rfft_q15 -- built here with g++ against libmsdr.so into a temporary directory and run against the golden answers."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "minimal-sdr_amd", "lib")


def build(tmp):
    exe = os.path.join(str(tmp), "test_cmsis_relink")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_cmsis_relink.cpp"),
                           os.path.join(ROOT, "minimal-sdr_amd", "host", "AudioStream.cpp"),
                           "-L" + LIBDIR, "-lmsdr", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_relink_program_builds_and_refuses_to_run_without_gpu(tmp_path):
    exe = build(tmp_path)
    out = subprocess.run([exe, "--no-gpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "no-gpu path: OK" in out.stdout


@pytest.mark.gpu
def test_relinked_sketch_sections_bit_exact(tmp_path, golden, orc):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
    import msdr
    exe = build(tmp_path)
    B, rewrite = 128, 3

    def put(name, a):
        np.ascontiguousarray(a, np.int16).tofile(os.path.join(str(tmp_path), name))

    # (a) FIR_I: the AM taps on the full-scale signal, rewritten in place before block 3; FIR_Q: the SSB Q taps on the noise signal
    ti, tq = golden["fir/taps_am102"], golden["fir/taps_ssb_q"]
    ti2 = msdr.calc_fir_coeffs(102, 2000)[:102]
    xi, xq = golden["fir/x_full"], golden["fir/x_noise"]
    want_i = golden["fir/am102_full_b128"].copy()
    _, after = orc.fir_q15_blocks(ti2, xi, B)          # the filter keeps its history across the rewrite: the new taps on the same stream
    want_i[rewrite * B:] = after[rewrite * B:]
    put("fir_taps_i.bin", ti)
    put("fir_taps_i2.bin", ti2)
    put("fir_taps_q.bin", tq)
    put("fir_x_i.bin", xi)
    put("fir_x_q.bin", xq)
    put("fir_want_i.bin", want_i)
    put("fir_want_q.bin", golden["fir/ssb_q_noise_b128"])
    put("fir_rewrite_block.bin", [rewrite])
    # (c) the spectrum transform
    put("fft_x.bin", golden["fft/x"])
    put("fft_out.bin", golden["fft/rfft128_out"])
    put("fft_work.bin", golden["fft/rfft128_work"])
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip().endswith("(c) arm_rfft_q15") and out.stdout.startswith("OK"), out.stdout
