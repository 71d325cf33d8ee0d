"""The S-meter's host side (msdr_chain_set_meter / msdr_chain_get_meter / msdr_meter_dbfs, MSDR_FLAVOUR_METER): declared in include/msdr.h,
exported by libmsdr.so, the flavour bit an enumerator that collides with no other, msdr_chain_config as every earlier build laid it out,
the Python mirror, and msdr_meter_dbfs against a numpy restatement of its formula.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
import msdr  # noqa: E402


def test_the_calls_are_declared_exported_and_mirrored(tmp_path):
    with open(os.path.join(ROOT, "include", "msdr.h")) as f:
        h = f.read()
    for decl in (r"^int msdr_chain_set_meter\(msdr_chain \*chain, void \*d_meter\);", r"^int msdr_chain_get_meter\(msdr_chain \*chain, void \*\*d_meter\);",
                 r"^double msdr_meter_dbfs\(double sum_sq, uint64_t n_out, double full_scale\);"):
        assert re.search(decl, h, re.M), decl
    assert re.search(r"^enum \{ MSDR_FLAVOUR_METER = 0x200000u \};", h, re.M)           # an enumerator: tests/test_abi.py counts the macros
    lib = os.path.join(ROOT, "minimal-sdr_amd", "lib", "libmsdr.so")
    out = subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True, text=True).stdout
    for sym in ("msdr_chain_set_meter", "msdr_chain_get_meter", "msdr_meter_dbfs"):
        assert re.search(r" T %s$" % sym, out, re.M), sym
    others = sorted(set(re.findall(r"MSDR_FLAVOUR_[A-Z0-9_]+", h)) - {"MSDR_FLAVOUR_METER", "MSDR_FLAVOUR_FOLD_PERIOD_SHIFT", "MSDR_FLAVOUR_FOLD_PERIOD"})
    assert len(others) >= 17, others
    src = os.path.join(str(tmp_path), "size.c")
    with open(src, "w") as f:
        f.write('#include <stdio.h>\n#include "msdr.h"\nint main(void) { printf("%zu %u %u\\n", sizeof(msdr_chain_config), (unsigned)MSDR_FLAVOUR_METER,\n'
                '    (unsigned)(' + " | ".join(others) + ' | (7u << MSDR_FLAVOUR_FOLD_PERIOD_SHIFT))); return 0; }\n')
    exe = os.path.join(str(tmp_path), "size")
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), "-o", exe, src])
    size, bit, rest = (int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split())
    assert size == C.sizeof(msdr.ChainConfig) == 264          # the struct as every earlier build laid it out (LP64)
    assert bit == msdr.FLAVOUR_METER == 0x200000
    assert not bit & rest, hex(rest)                         # disjoint from every other flavour bit and from the fold period's field
    assert callable(msdr.Chain.set_meter) and callable(msdr.Chain.meter) and callable(msdr.meter_dbfs)


def test_meter_dbfs_is_its_formula():
    rng = np.random.default_rng(77)
    for _ in range(20):
        s = float(10.0 ** rng.uniform(0.0, 19.0))
        n = int(rng.integers(1, 1 << 31))
        fs = float(rng.choice([32768.0, 1.0, 32768.0 / 32768.0 * 0.5, 32768.0 * 3.0]))
        want = 10.0 * np.log10((s / n) / (fs * fs / 4.0))
        assert abs(msdr.meter_dbfs(s, n, fs) - want) <= 1e-12 * max(1.0, abs(want)), (s, n, fs)
    # a full-scale carrier behind a unity-gain filter: I^2 + Q^2 = A^2 / 4 per output is 0 dBFS, a tenth of the amplitude -20
    assert abs(msdr.meter_dbfs(128 * 32768.0 ** 2 / 4.0, 128)) < 1e-12
    assert abs(msdr.meter_dbfs(128 * 3276.8 ** 2 / 4.0, 128) + 20.0) < 1e-9
    assert abs(msdr.meter_dbfs(1000 * 0.25, 1000, 1.0)) < 1e-12
    assert msdr.meter_dbfs(0.0, 128) == -np.inf
    assert msdr.meter_dbfs(-1.0, 128) == -np.inf
    assert msdr.meter_dbfs(1.0e9, 0) == -np.inf


def test_a_null_chain_is_an_argument_error():
    lib = msdr.load_library()
    p = C.c_void_p()
    assert lib.msdr_chain_set_meter(None, None) == msdr.STATUS_ARGUMENT_ERROR
    assert lib.msdr_chain_get_meter(None, C.byref(p)) == msdr.STATUS_ARGUMENT_ERROR
