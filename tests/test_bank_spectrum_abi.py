"""msdr_chain_set_spectrum, the 64-point complex FFT stage and msdr_spectrum_dbfs through the layers: exported by libmsdr.so, declared in
include/msdr.h, wrapped by python/msdr.py; MSDR_FLAVOUR_SPECTRUM one bit that no other flavour value has; the dBFS convention.  CPU only."""
import ctypes
import math
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "msdr.h")
LIB = os.path.join(ROOT, "minimal-sdr_amd", "lib", "libmsdr.so")
DECLS = ("int msdr_cfft64_q15(msdr_ctx *ctx, const q15_t *d_pairs, uint64_t stride_pairs, q15_t *d_bins, uint32_t *d_power, uint32_t nfft);",
         "int msdr_cfft64_f32(msdr_ctx *ctx, const float *d_pairs, uint64_t stride_pairs, float *d_bins, float *d_power, uint32_t nfft);",
         "int msdr_chain_set_spectrum(msdr_chain *chain, void *d_bins, void *d_power, uint32_t every);",
         "int msdr_chain_get_spectrum(msdr_chain *chain, void **d_bins, void **d_power, uint32_t *every, uint64_t *drawn);",
         "double msdr_spectrum_dbfs(double power, double full_scale);")
ARG = -1          # MSDR_STATUS_ARGUMENT_ERROR


def header():
    with open(HEADER) as f:
        return f.read()


def wrapper():
    sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
    import msdr
    return msdr


def test_the_symbols_are_exported_and_declared_with_their_argument_types():
    lib = ctypes.CDLL(LIB)
    text = header()
    for d in DECLS:
        assert d in text, d
        assert hasattr(lib, re.search(r"(msdr_\w+)\(", d).group(1)), d
    assert int(re.search(r"#define\s+MSDR_SPECTRUM_BINS\s+(\d+)", text).group(1)) == 64


def test_a_null_chain_is_refused_without_a_device():
    lib = ctypes.CDLL(LIB)
    drawn = (ctypes.c_uint64 * 1)(7)
    assert lib.msdr_chain_set_spectrum(None, None, None, 0) == ARG
    assert lib.msdr_chain_get_spectrum(None, None, None, None, drawn) == ARG and drawn[0] == 7


def test_dbfs_is_the_meters_convention():
    lib = ctypes.CDLL(LIB)
    lib.msdr_spectrum_dbfs.restype = ctypes.c_double
    lib.msdr_spectrum_dbfs.argtypes = [ctypes.c_double, ctypes.c_double]
    assert lib.msdr_spectrum_dbfs(2.0 ** 28, 32768.0) == 0.0          # (A / 2)^2 of a full-scale real carrier
    assert lib.msdr_spectrum_dbfs(0.0, 32768.0) == -math.inf and lib.msdr_spectrum_dbfs(-1.0, 32768.0) == -math.inf
    assert abs(lib.msdr_spectrum_dbfs(2.0 ** 28 / 100.0, 32768.0) + 20.0) < 1e-12
    assert abs(lib.msdr_spectrum_dbfs(0.25 * 0.5 ** 2, 0.5) - 0.0) < 1e-12          # fp32 chain, in_scale = 2^-16
    msdr = wrapper()
    assert msdr.spectrum_dbfs(2.0 ** 28) == 0.0 and msdr.spectrum_dbfs(0.0) == -math.inf


def test_the_python_wrapper_has_its_methods_and_constants():
    msdr = wrapper()
    for m in ("set_spectrum", "spectrum"):
        assert callable(getattr(msdr.Chain, m)), m
    for m in ("cfft64_q15", "cfft64_f32"):
        assert callable(getattr(msdr.Context, m)), m
    assert msdr.SPECTRUM_BINS == 64
    assert msdr.FLAVOUR_SPECTRUM == int(re.search(r"enum \{ MSDR_FLAVOUR_SPECTRUM = (0x[0-9a-fA-F]+)u \};", header()).group(1), 16) == 0x4000000


def test_the_flavour_value_is_an_enumerator_and_one_bit_of_its_own():
    text = header()
    assert not re.search(r"#define\s+MSDR_FLAVOUR_SPECTRUM", text)
    vals = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"(MSDR_FLAVOUR_[A-Z0-9_]+)\s*=?\s+(0x[0-9a-fA-F]+)u", text)}
    g = vals.pop("MSDR_FLAVOUR_SPECTRUM")
    assert len(vals) >= 13, vals
    assert g and g & (g - 1) == 0
    for k, v in vals.items():
        assert v != g and not (v & g), k
    assert not (g & (7 << 12))          # (MSDR_FLAVOUR_FOLD_PERIOD's field)
