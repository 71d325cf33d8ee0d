"""The phase-accumulator oscillator's host side (minimal-sdr_amd/csrc/msdr_nco.h, msdr_nco_step / msdr_nco_table / msdr_nco_q15): the table,
the interpolated sine against a numpy restatement of include/msdr.h's formulas (written here, not taken from the library), the step rule, the
agreement with 128-entry tables on their grid, a stand-alone sanitised program that walks every (i, f) pair, and the Python setter's argument
checks.  No GPU needed."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
import msdr  # noqa: E402


def table_model():
    t = np.round(32767 * np.sin(2 * np.pi * np.arange(1025) / 1024)).astype(np.int64)
    t[1024] = 0
    return t


def sinq_model(phi):
    """include/msdr.h, msdr_nco_q15: i = phi >> 22, f = (phi >> 6) & 0xFFFF, T[i] + (((T[i + 1] - T[i]) * f + 32768) >> 16)"""
    t = table_model()
    phi = np.asarray(phi, np.uint64) & np.uint64(0xFFFFFFFF)
    i = (phi >> np.uint64(22)).astype(np.int64)
    f = ((phi >> np.uint64(6)) & np.uint64(0xFFFF)).astype(np.int64)
    return t[i] + (((t[i + 1] - t[i]) * f + 32768) >> 16)          # (numpy's >> on int64 is arithmetic)


def cosq_model(phi):
    return sinq_model((np.asarray(phi, np.uint64) + np.uint64(0x40000000)) & np.uint64(0xFFFFFFFF))


def test_the_table_is_the_rounded_sine():
    t = msdr.nco_table()
    assert t.dtype == np.int16 and t.shape == (1025,)
    assert np.array_equal(t, np.round(32767 * np.sin(2 * np.pi * np.arange(1025) / 1024)))
    assert t[1024] == 0 and np.abs(np.diff(t.astype(np.int32))).max() <= 201


def test_nco_q15_equals_the_numpy_restatement():
    rng = np.random.default_rng(20240607)
    phi = np.concatenate([rng.integers(0, 1 << 32, 1000000, dtype=np.uint64).astype(np.uint32),
                          np.array([0, (1 << 22) - 1, 1 << 22, 1 << 30, 1 << 31, (1 << 32) - 1], np.uint32)])
    s, c = msdr.nco_q15(phi)
    assert s.dtype == np.int16 and c.dtype == np.int16
    assert np.array_equal(s, sinq_model(phi)) and np.array_equal(c, cosq_model(phi))
    assert s.min() >= -32767 and s.max() <= 32767
    err = np.abs(s.astype(np.float64) - 32767 * np.sin(2 * np.pi * phi.astype(np.float64) / 2.0 ** 32))
    assert err.max() <= 1.16, err.max()                                   # 0.5 + 0.5 + 32767 (2 pi / 1024)^2 / 8 = 1.154, and the 6 dropped bits


def test_either_output_of_nco_q15_may_be_null():
    import ctypes as C
    lib = msdr.load_library()
    phi = np.array([123456789, 0xC0000000], np.uint32)
    s, c = np.zeros(2, np.int16), np.zeros(2, np.int16)
    lib.msdr_nco_q15(phi.ctypes.data_as(C.c_void_p), C.c_size_t(2), s.ctypes.data_as(C.c_void_p), None)
    lib.msdr_nco_q15(phi.ctypes.data_as(C.c_void_p), C.c_size_t(2), None, c.ctypes.data_as(C.c_void_p))
    assert np.array_equal(s, sinq_model(phi)) and np.array_equal(c, cosq_model(phi))


def test_nco_step():
    assert msdr.nco_step(6000.0, 24000.0) == 0x40000000
    assert msdr.nco_step(-6000.0, 24000.0) == 0xC0000000
    for k in range(128):
        assert msdr.nco_step(k * 24000.0 / 128, 24000.0) == k << 25, k
    assert msdr.nco_step(1.0, 24000.0) == round(2 ** 32 / 24000.0)


def test_on_the_128_grid_the_oscillator_is_the_rounded_table():
    n = np.arange(128, dtype=np.uint64)
    for k in range(128):
        phi = ((n * np.uint64(k << 25)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        s, c = msdr.nco_q15(phi)
        assert np.array_equal(s, np.round(32767 * np.sin(2 * np.pi * k * np.arange(128) / 128))), k
        assert np.array_equal(c, np.round(32767 * np.cos(2 * np.pi * k * np.arange(128) / 128))), k


def test_stand_alone_sanitised_program_walks_every_pair(tmp_path):
    """tests/cpp/nco_host_check.cpp: its own main over msdr_nco.h, built with the address and undefined-behaviour sanitizers and run directly"""
    exe = os.path.join(str(tmp_path), "nco_host_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "minimal-sdr_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "nco_host_check.cpp")],
                   check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("OK"), (r.returncode, r.stdout, r.stderr)
    assert float(r.stdout.split()[2]) <= 1.16


def test_set_nco_channels_refuses_malformed_arrays_before_any_library_call():
    c = msdr.Chain.__new__(msdr.Chain)                    # an object that never reaches the library: no ctx, no handle
    try:
        good = np.arange(3, dtype=np.uint32)
        for bad in (np.zeros(3, np.float32), np.zeros((3, 1), np.uint32), np.zeros(0, np.uint32), np.array([-1, 0, 1]), np.array([0, 1 << 32, 1]),
                    np.zeros(3, np.complex64)):
            with pytest.raises(ValueError):
                c.set_nco_channels(0, bad)
            with pytest.raises(ValueError):
                c.set_nco_channels(0, good, bad)
        with pytest.raises(ValueError):                   # both well-formed, not the same length
            c.set_nco_channels(0, good, np.zeros(2, np.uint32))
        with pytest.raises(AttributeError):               # well-formed arrays get as far as the (missing) library handle
            c.set_nco_channels(0, good)
        with pytest.raises(AttributeError):
            c.set_nco_channels(0, good, good)
    finally:
        c.h = None
