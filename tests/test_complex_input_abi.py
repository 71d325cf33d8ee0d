"""msdr_chain_set_complex_input / msdr_chain_get_complex_input through the layers: exported by libmsdr.so, declared in include/msdr.h, wrapped
by python/msdr.py, and MSDR_FLAVOUR_COMPLEX_IN one bit that no other flavour value has.  CPU only."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "msdr.h")
LIB = os.path.join(ROOT, "minimal-sdr_amd", "lib", "libmsdr.so")
NAMES = ("msdr_chain_set_complex_input", "msdr_chain_get_complex_input")


def header():
    with open(HEADER) as f:
        return f.read()


def test_the_two_symbols_are_exported_and_declared():
    lib = ctypes.CDLL(LIB)
    text = header()
    for n in NAMES:
        assert hasattr(lib, n), n
    assert re.search(r"int msdr_chain_set_complex_input\(msdr_chain \*chain, int on, int dir\);", text)
    assert re.search(r"int msdr_chain_get_complex_input\(msdr_chain \*chain, int \*on, int \*dir\);", text)
    # a NULL chain is refused without a device
    assert lib.msdr_chain_set_complex_input(None, 1, 0) != 0 and lib.msdr_chain_get_complex_input(None, None, None) != 0


def test_the_python_wrapper_has_the_two_methods():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
    import msdr
    assert callable(msdr.Chain.set_complex_input) and callable(msdr.Chain.complex_input)
    assert msdr.FLAVOUR_COMPLEX_IN == int(re.search(r"MSDR_FLAVOUR_COMPLEX_IN = (0x[0-9a-fA-F]+)u", header()).group(1), 16)


def test_the_flavour_value_is_one_bit_of_its_own():
    vals = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"(MSDR_FLAVOUR_[A-Z0-9_]+)\s*=?\s+(0x[0-9a-fA-F]+)u", header())}
    cx = vals.pop("MSDR_FLAVOUR_COMPLEX_IN")
    assert len(vals) >= 10, vals
    assert cx and cx & (cx - 1) == 0
    for k, v in vals.items():
        assert v != cx and not (v & cx), k


def test_the_node_program_builds_with_werror_and_its_no_gpu_path_runs(tmp_path):
    import subprocess
    from test_gpu_complex_input_nodes import build
    out = subprocess.run([build(tmp_path), "--no-gpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "no-gpu path: OK" in out.stdout, out.stdout + out.stderr
