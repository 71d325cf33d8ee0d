"""msdr_chain_set_input_rows, the parts that need no GPU: the declaration and the export, the flavour bit as an enumerator beside the
MSDR_FLAVOUR_ macros, the size of the config struct, the Python wrapper's refusals, and the --no-gpu path of tests/cpp/test_input_rows.cpp."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
import msdr  # noqa: E402

HEADER = open(os.path.join(ROOT, "include", "msdr.h")).read()
LIBDIR = os.path.join(ROOT, "minimal-sdr_amd", "lib")


def test_the_call_is_declared_and_exported():
    assert re.search(r"int\s+msdr_chain_set_input_rows\s*\(\s*msdr_chain\s*\*\s*chain\s*,\s*uint32_t\s+n_inputs\s*,\s*const\s+uint32_t\s*\*\s*input_row\s*\)\s*;", HEADER)
    lib = msdr.load_library()
    assert hasattr(lib, "msdr_chain_set_input_rows")
    assert lib.msdr_chain_set_input_rows.argtypes == [C.c_void_p, C.c_uint32, C.c_void_p]
    assert lib.msdr_chain_set_input_rows(None, C.c_uint32(0), None) == msdr.STATUS_ARGUMENT_ERROR          # a NULL chain, before any device is looked for


def test_the_flavour_bit_is_an_enumerator_that_overlaps_no_other():
    m = re.search(r"enum\s*\{\s*MSDR_FLAVOUR_SHARED_IF\s*=\s*(0x[0-9a-fA-F]+)u?\s*\}\s*;", HEADER)
    assert m and int(m.group(1), 16) == 0x40000
    assert not re.search(r"#\s*define\s+MSDR_FLAVOUR_SHARED_IF\b", HEADER)
    others = {}
    for name, val in re.findall(r"#\s*define\s+(MSDR_FLAVOUR_[A-Z0-9_]+)\s+(0x[0-9a-fA-F]+)u", HEADER):
        others[name] = int(val, 16)
    for name, val in re.findall(r"enum\s*\{\s*(MSDR_FLAVOUR_[A-Z0-9_]+)\s*=\s*(0x[0-9a-fA-F]+)u?\s*\}", HEADER):
        others[name] = int(val, 16)
    assert len(others) >= 16 and others.pop("MSDR_FLAVOUR_SHARED_IF") == 0x40000
    for name, val in others.items():
        assert not val & 0x40000, name
    assert not (7 << 12) & 0x40000          # MSDR_FLAVOUR_FOLD_PERIOD's three bits
    assert msdr.FLAVOUR_SHARED_IF == 0x40000


def test_the_config_struct_keeps_its_size(tmp_path):
    assert C.sizeof(msdr.ChainConfig) == 264          # the binding's mirror ...
    src, exe = os.path.join(str(tmp_path), "size.c"), os.path.join(str(tmp_path), "size")
    with open(src, "w") as f:                         # ... and the header itself, as a C compiler lays it out
        f.write('#include <stdio.h>\n#include "msdr.h"\nint main(void) { printf("%zu\\n", sizeof(msdr_chain_config)); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe, src])
    assert int(subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout) == 264


def test_the_python_wrapper_refuses_malformed_arrays_before_any_library_call():
    c = msdr.Chain.__new__(msdr.Chain)                    # an object that never reaches the library: no ctx, no handle
    c.channels = 9
    good = np.array([2, 0, 0, 1, 2, 2, 1, 0, 2])
    try:
        for bad in (good[:8], np.zeros(10, np.int32), good.reshape(3, 3), good.reshape(9, 1), good.astype(np.float32), good.astype(bool).astype(object),
                    np.array([2, 0, 0, 1, -1, 2, 1, 0, 2]), np.zeros(0, np.int32)):
            with pytest.raises(ValueError):
                c.set_input_rows(bad)
        for ni in (2, 0, -1, 2.5):                          # an entry >= n_inputs; no rows at all
            with pytest.raises(ValueError):
                c.set_input_rows(good, n_inputs=ni)
    except AttributeError as e:                             # the wrapper got as far as self.ctx: it did not refuse
        pytest.fail("a malformed array reached the library call: %s" % e)
    with pytest.raises(AttributeError):                     # ... and what is well-formed does go on to the library
        c.set_input_rows(good)
    with pytest.raises(AttributeError):
        c.set_input_rows(good.astype(np.uint8), n_inputs=64)
    with pytest.raises(AttributeError):
        c.set_input_rows(None)


def test_the_cpp_program_builds_and_refuses_bad_arguments_without_a_gpu(tmp_path):
    exe = os.path.join(str(tmp_path), "test_input_rows")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_input_rows.cpp"),
                           os.path.join(ROOT, "minimal-sdr_amd", "host", "AudioStream.cpp"),
                           "-L" + LIBDIR, "-lmsdr", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, "--no-gpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "no-gpu path: OK" in out.stdout
