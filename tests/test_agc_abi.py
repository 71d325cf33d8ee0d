"""msdr_chain_set_gain / set_gain_channels / set_agc / get_agc through the layers: exported by libmsdr.so, declared in include/msdr.h, wrapped by
python/msdr.py, and MSDR_FLAVOUR_GAIN one bit that no other flavour value has.  CPU only."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "msdr.h")
LIB = os.path.join(ROOT, "minimal-sdr_amd", "lib", "libmsdr.so")
NAMES = ("msdr_chain_set_gain", "msdr_chain_get_gain", "msdr_chain_set_gain_channels", "msdr_chain_set_agc", "msdr_chain_get_agc")
ARG = -1          # MSDR_STATUS_ARGUMENT_ERROR


def header():
    with open(HEADER) as f:
        return f.read()


def test_the_symbols_are_exported_and_declared():
    lib = ctypes.CDLL(LIB)
    text = header()
    for n in NAMES:
        assert hasattr(lib, n), n
    assert re.search(r"int msdr_chain_set_gain\(msdr_chain \*chain, int on\);", text)
    assert re.search(r"int msdr_chain_set_gain_channels\(msdr_chain \*chain, uint32_t first_channel, uint32_t count, const float \*gain\);", text)
    assert re.search(r"int msdr_chain_set_agc\(msdr_chain \*chain, const int32_t \*agc_on, int32_t agc_on_all\);", text)
    assert re.search(r"#define MSDR_AGC_STATE_WORDS 32u", text)
    assert re.search(r"int msdr_chain_get_agc\(msdr_chain \*chain, uint32_t channel, int32_t state\[MSDR_AGC_STATE_WORDS\]\);", text)
    assert int(re.search(r"MSDR_STATUS_ARGUMENT_ERROR\s*=\s*(-?\d+)", text).group(1)) == ARG


def test_a_null_chain_is_refused_without_a_device():
    lib = ctypes.CDLL(LIB)
    state = (ctypes.c_int32 * 32)(*([7] * 32))
    gain = (ctypes.c_float * 1)(2.0)
    on = (ctypes.c_int32 * 1)(1)
    assert lib.msdr_chain_set_gain(None, 1) == ARG and lib.msdr_chain_set_gain(None, 0) == ARG
    assert lib.msdr_chain_get_gain(None, None) == ARG
    assert lib.msdr_chain_set_gain_channels(None, 0, 1, gain) == ARG and lib.msdr_chain_set_gain_channels(None, 0, 0, None) == ARG
    assert lib.msdr_chain_set_agc(None, on, 0) == ARG and lib.msdr_chain_set_agc(None, None, 1) == ARG
    assert lib.msdr_chain_get_agc(None, 0, state) == ARG and list(state) == [7] * 32


def test_the_python_wrapper_has_its_methods():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
    import msdr
    for m in ("set_gain", "gain", "set_gain_channels", "set_agc", "agc_state"):
        assert callable(getattr(msdr.Chain, m)), m
    assert msdr.FLAVOUR_GAIN == int(re.search(r"MSDR_FLAVOUR_GAIN = (0x[0-9a-fA-F]+)u", header()).group(1), 16) == 0x1000000
    assert msdr.AGC_STATE_WORDS == 32


def test_the_flavour_value_is_one_bit_of_its_own():
    vals = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"(MSDR_FLAVOUR_[A-Z0-9_]+)\s*=?\s+(0x[0-9a-fA-F]+)u", header())}
    g = vals.pop("MSDR_FLAVOUR_GAIN")
    assert len(vals) >= 11, vals
    assert g and g & (g - 1) == 0
    for k, v in vals.items():
        assert v != g and not (v & g), k


def test_the_node_program_builds_with_werror_and_its_no_gpu_path_runs(tmp_path):
    import subprocess
    from test_gpu_agc_nodes import build
    out = subprocess.run([build(tmp_path), "--no-gpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "no-gpu path: OK" in out.stdout, out.stdout + out.stderr
