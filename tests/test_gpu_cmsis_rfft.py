"""include/msdr_cmsis.h on the GPU: arm_rfft_init_q15 / arm_rfft_q15 (arm_math.h:2146-2166) as UI.cpp:523, 550 call them.  Like CMSIS,
arm_rfft_q15 transforms pSrc in place (arm_rfft_q15.c:103-107): FFT_out must equal the reference's answers and the clobbered pSrc its
work buffer, both pinned in tests/golden (fft/rfft128_out, fft/rfft128_work; ref_live.npz rfft128/out, rfft128/work)."""
import ctypes as C

import numpy as np
import pytest

import reflive
from gpuhelp import ctx, msdr  # noqa: F401

pytestmark = pytest.mark.gpu


class CfftQ15(C.Structure):           # arm_math.h:2095-2101
    _fields_ = [("fftLen", C.c_uint16), ("pTwiddle", C.c_void_p), ("pBitRevTable", C.c_void_p), ("bitRevLength", C.c_uint16)]


class RfftQ15(C.Structure):           # arm_math.h:2146-2155
    _fields_ = [("fftLenReal", C.c_uint32), ("ifftFlagR", C.c_uint8), ("bitReverseFlagR", C.c_uint8), ("twidCoefRModifier", C.c_uint32),
                ("pTwiddleAReal", C.c_void_p), ("pTwiddleBReal", C.c_void_p), ("pCfft", C.POINTER(CfftQ15))]


def lib_of(ctx):
    lib = ctx.lib
    lib.msdr_arm_rfft_init_q15.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
    lib.msdr_arm_rfft_q15.argtypes, lib.msdr_arm_rfft_q15.restype = [C.c_void_p, C.c_void_p, C.c_void_p], None
    lib.msdr_cmsis_bind.argtypes = lib.msdr_cmsis_bind_host.argtypes = [C.c_void_p, C.c_uint32]
    return lib


@pytest.fixture
def unbind(ctx):
    yield
    lib_of(ctx).msdr_cmsis_bind(None, 0)


def fft_instance(lib):
    S = RfftQ15()
    assert lib.msdr_arm_rfft_init_q15(C.byref(S), 128, 0, 1) == 0           # initSpectrum(), UI.cpp:523
    return S


def test_rfft_init_status_and_fields(ctx, golden):
    lib = lib_of(ctx)
    S = fft_instance(lib)
    assert (S.fftLenReal, S.ifftFlagR, S.bitReverseFlagR, S.twidCoefRModifier) == (128, 0, 1, 64)     # arm_rfft_init_q15.c:2166-2209
    assert S.pTwiddleAReal is None and S.pTwiddleBReal is None
    cf = S.pCfft.contents
    assert (cf.fftLen, cf.pBitRevTable, cf.bitRevLength) == (64, None, 0)
    tw = np.ctypeslib.as_array(C.cast(cf.pTwiddle, C.POINTER(C.c_int16)), (96,))
    assert np.array_equal(tw, golden["fft/twiddleCoef_64_q15"])
    # lengths CMSIS does not know: ARGUMENT_ERROR, the modifier and pCfft untouched (the switch's default, :2217-2220)
    for n in (0, 16, 100, 129, 16384):
        T = RfftQ15(7, 9, 9, 12345)
        assert lib.msdr_arm_rfft_init_q15(C.byref(T), n, 0, 1) == -1, n
        assert (T.fftLenReal, T.ifftFlagR, T.bitReverseFlagR, T.twidCoefRModifier) == (n & 0xffff, 0, 1, 12345)
    # CMSIS-valid, not built here: LENGTH_ERROR with the CMSIS modifier and no complex-FFT instance
    for n, ifft, rev in ((32, 0, 1), (64, 0, 1), (256, 0, 1), (8192, 0, 1), (128, 1, 1), (128, 0, 0)):
        T = RfftQ15()
        assert lib.msdr_arm_rfft_init_q15(C.byref(T), n, ifft, rev) == -2, (n, ifft, rev)
        assert T.twidCoefRModifier == 8192 // n and not T.pCfft, (n, ifft, rev)
    # the length is stored as uint16_t before the switch, as there
    T = RfftQ15()
    assert lib.msdr_arm_rfft_init_q15(C.byref(T), 65536 + 128, 0, 1) == 0 and T.fftLenReal == 128


def test_rfft_device_binding_golden(ctx, unbind, golden):
    lib = lib_of(ctx)
    x = golden["fft/x"]
    nfft = x.shape[0]
    assert lib.msdr_cmsis_bind(ctx.h, nfft) == 0
    S = fft_instance(lib)
    d_src, d_out = ctx.to_device(x), ctx.array((nfft, 256), np.int16).fill(0x33)
    lib.msdr_arm_rfft_q15(C.byref(S), d_src.ptr, d_out.ptr)
    assert np.array_equal(d_out.download(), golden["fft/rfft128_out"])
    assert np.array_equal(d_src.download(), golden["fft/rfft128_work"])


def test_rfft_host_binding_golden(ctx, unbind, golden):
    lib = lib_of(ctx)
    x = golden["fft/x"]
    nfft = x.shape[0]
    S = fft_instance(lib)
    assert lib.msdr_cmsis_bind_host(ctx.h, nfft) == 0
    src, out = x.copy(), np.zeros((nfft, 256), np.int16)
    lib.msdr_arm_rfft_q15(C.byref(S), src.ctypes.data, out.ctypes.data)
    assert np.array_equal(out, golden["fft/rfft128_out"])
    assert np.array_equal(src, golden["fft/rfft128_work"])
    # the sketch's shape: one channel, one transform per call
    assert lib.msdr_cmsis_bind_host(ctx.h, 1) == 0
    for f in (0, 5, 17, nfft - 1):
        src, out = x[f].copy(), np.zeros(256, np.int16)
        lib.msdr_arm_rfft_q15(C.byref(S), src.ctypes.data, out.ctypes.data)
        assert np.array_equal(out, golden["fft/rfft128_out"][f]) and np.array_equal(src, golden["fft/rfft128_work"][f]), f


def test_rfft_matches_reference_live_answers(ctx, unbind):
    lib = lib_of(ctx)
    S = fft_instance(lib)
    for d in reflive.answers("rfft128"):
        x = d["x"]
        assert lib.msdr_cmsis_bind(ctx.h, x.shape[0]) == 0
        d_src, d_out = ctx.to_device(x), ctx.array((x.shape[0], 256), np.int16)
        lib.msdr_arm_rfft_q15(C.byref(S), d_src.ptr, d_out.ptr)
        assert np.array_equal(d_out.download(), d["out"])
        assert np.array_equal(d_src.download(), d["work"])


def test_rfft_refusals_write_nothing(ctx, unbind, golden):
    lib = lib_of(ctx)
    x = golden["fft/x"][:4]
    bad = RfftQ15()
    assert lib.msdr_arm_rfft_init_q15(C.byref(bad), 256, 0, 1) == -2
    assert lib.msdr_cmsis_bind(ctx.h, 4) == 0
    d_src, d_out = ctx.to_device(x), ctx.to_device(np.full((4, 256), 99, np.int16))
    lib.msdr_arm_rfft_q15(C.byref(bad), d_src.ptr, d_out.ptr)                       # an instance that did not initialise
    assert np.array_equal(d_src.download(), x) and (d_out.download() == 99).all()
    assert "arm_rfft_init_q15" in lib.msdr_last_error().decode()
    S = fft_instance(lib)
    host_out = np.full((4, 256), 99, np.int16)
    lib.msdr_arm_rfft_q15(C.byref(S), d_src.ptr, host_out.ctypes.data)               # host pDst under the device binding
    assert np.array_equal(d_src.download(), x) and (host_out == 99).all() and lib.msdr_last_error().decode()
    big = ctx.to_device(np.concatenate([np.zeros(1, np.int16), x.reshape(-1), np.zeros(7, np.int16)]))
    lib.msdr_arm_rfft_q15(C.byref(S), big.ptr + 2, d_out.ptr)                          # an unaligned device pSrc is refused
    assert (d_out.download() == 99).all() and "aligned" in lib.msdr_last_error().decode()
    assert lib.msdr_cmsis_bind_host(ctx.h, 4) == 0
    lib.msdr_arm_rfft_q15(C.byref(S), d_src.ptr, host_out.ctypes.data)               # device pSrc under the host binding
    assert np.array_equal(d_src.download(), x) and (host_out == 99).all() and "device pointer" in lib.msdr_last_error().decode()
    assert lib.msdr_cmsis_bind(None, 0) == 0
    src = x.copy()
    lib.msdr_arm_rfft_q15(C.byref(S), src.ctypes.data, host_out.ctypes.data)          # unbound
    assert np.array_equal(src, x) and (host_out == 99).all() and "no context bound" in lib.msdr_last_error().decode()


def test_c_abi_inplace_and_read_only_forms(ctx, golden):
    """msdr_rfft128_q15 still leaves d_src untouched; msdr_rfft128_q15_inplace writes the work buffer, at a padded stride too, and does so
    even with both other outputs NULL."""
    x = golden["fft/x"]
    nfft, stride = x.shape[0], 136
    buf = np.full((nfft, stride), 555, np.int16)
    buf[:, :128] = x
    d = ctx.to_device(buf)
    o, c = ctx.array((nfft, 256), np.int16), ctx.array((nfft, 128), np.uint8)
    msdr.rfft128_q15(ctx, d, stride, nfft, o, c)
    assert np.array_equal(d.download(), buf)
    assert np.array_equal(o.download(), golden["fft/rfft128_out"])
    o2, c2 = ctx.array((nfft, 256), np.int16), ctx.array((nfft, 128), np.uint8)
    msdr.rfft128_q15_inplace(ctx, d, stride, nfft, o2, c2)
    got = d.download()
    assert np.array_equal(got[:, :128], golden["fft/rfft128_work"]) and (got[:, 128:] == 555).all()
    assert np.array_equal(o2.download(), golden["fft/rfft128_out"]) and np.array_equal(c2.download(), c.download())
    d3 = ctx.to_device(buf)
    msdr.rfft128_q15_inplace(ctx, d3, stride, nfft)
    assert np.array_equal(d3.download()[:, :128], golden["fft/rfft128_work"])


def test_c_abi_inplace_many_batches(ctx, orc):
    """More transforms than the launch has workgroups x 16: a wave walks several batches, prefetching the next one's samples while it
    writes this one's work buffer."""
    nfft = 8192 * 16 + 16 * 3 + 5
    rng = np.random.default_rng(31)
    x = rng.integers(-32768, 32768, (nfft, 128)).astype(np.int16)
    d, o = ctx.to_device(x), ctx.array((nfft, 256), np.int16)
    msdr.rfft128_q15_inplace(ctx, d, 128, nfft, o)
    got, out = d.download(), o.download()
    for f in list(range(0, 20)) + list(range(131072 - 10, nfft)):
        want, work = orc.rfft128_q15(x[f])
        assert np.array_equal(out[f], want) and np.array_equal(got[f], work), f
