"""ctypes binding of the C ABI in include/msdr.h (minimal-sdr_amd/lib/libmsdr.so).

This is the stub a Python caller binds; the product is the shared library.  Used by tests/ and
bench.py.  It never falls back to a CPU implementation: if the library or a gfx950 device is
missing, construction raises."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libmsdr.so")

MODE_SYNCAM, MODE_AM, MODE_LSB, MODE_USB, MODE_CW = 0, 1, 2, 3, 4
SQRT_F32, SQRT_Q31 = 0, 1
MIXER_FS4, MIXER_NCO = 0, 1
ARITH_Q15, ARITH_F32 = 0, 1
BQ_LOWPASS, BQ_HIGHPASS, BQ_BANDPASS, BQ_NOTCH, BQ_LOWSHELF, BQ_HIGHSHELF = range(6)
AUDIO_SAMPLE_RATE_EXACT = 44117.64706
MAX_TAPSETS = 8
CHAIN_NO_TAP_FOLDING = 1
CHAIN_NO_MFMA = 8
CHAIN_SYNCAM_PLL = 32
CHAIN_FOLD_ANY_PERIOD = 64
CHAIN_OUT_I16 = 128
# msdr_chain_info.flavour (include/msdr.h: MSDR_FLAVOUR_*)
FLAVOUR_SSB_UNITS, FLAVOUR_ENV_UNITS, FLAVOUR_SSB_FOLD, FLAVOUR_ENV_FOLD = 0x1, 0x2, 0x4, 0x8
FLAVOUR_FULL_RATE, FLAVOUR_COMPACT, FLAVOUR_SHARED_IQ, FLAVOUR_AMTR = 0x10, 0x20, 0x40, 0x80
FLAVOUR_BLOCK, FLAVOUR_VALU_FOLD, FLAVOUR_SEQ_CASCADE, FLAVOUR_SEGMENTED = 0x100, 0x200, 0x400, 0x800
FLAVOUR_FOLD_PERIOD_SHIFT = 12
FLAVOUR_TAPS_PC = 0x8000
FLAVOUR_CASCADE_PC = 0x10000
FLAVOUR_OSC_PC = 0x20000
FLAVOUR_SHARED_IF = 0x40000
FLAVOUR_NCO_PC = 0x80000
FLAVOUR_DECIMATED = 0x100000
FLAVOUR_METER = 0x200000
FLAVOUR_IQ_OUT = 0x400000
FLAVOUR_COMPLEX_IN = 0x800000
FLAVOUR_GAIN = 0x1000000
FLAVOUR_BANK_POST = 0x2000000
FLAVOUR_SPECTRUM = 0x4000000
FLAVOUR_PREFILTER = 0x8000000
SPECTRUM_BINS = 64
AGC_STATE_WORDS = 32
MAX_DECIMATION_Q15, MAX_DECIMATION_F32 = 60, 59
FE_DCBLOCK, FE_AMP, FE_AGC, FE_ALL = 1, 2, 4, 7

STATUS_ARGUMENT_ERROR, STATUS_LENGTH_ERROR, STATUS_NO_DEVICE = -1, -2, -100

_p = C.c_void_p


class MsdrError(RuntimeError):
    def __init__(self, status, text):
        super().__init__("msdr status %d: %s" % (status, text))
        self.status = status


class ChainConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("arith", C.c_int32), ("channels", C.c_uint32), ("mixer", C.c_int32),
                ("num_taps", C.c_uint32), ("num_tapsets", C.c_uint32),
                ("coeffs_i", _p * MAX_TAPSETS), ("coeffs_q", _p * MAX_TAPSETS),
                ("default_mode", C.c_int32), ("mode", _p), ("tapset", _p), ("sqrt_kind", C.c_int32),
                ("osc_len", C.c_uint32), ("osc_i", _p), ("osc_q", _p),
                ("in_scale", C.c_float), ("num_biquad_stages", C.c_uint32), ("biquad_coeffs", _p),
                ("num_biquad_nodes", C.c_uint32), ("node_stages", C.c_uint32 * 2), ("node_coefs", _p * 2),
                ("time_segments", C.c_uint32), ("biquad_warmup", C.c_uint32), ("flags", C.c_uint32)]


class ChainInfo(C.Structure):
    _fields_ = [("kernel", C.c_char * 64), ("grid", C.c_uint32), ("block", C.c_uint32), ("lds_bytes", C.c_uint32),
                ("time_segments", C.c_uint32), ("warmup", C.c_uint32), ("tile", C.c_uint32),
                ("taps_padded", C.c_uint32), ("mfma_ksteps", C.c_uint32), ("env_scan", C.c_uint32), ("flavour", C.c_uint32)]


_lib = None


def load_library(path=None):
    """Load libmsdr.so (no GPU needed to load it or to use the host-side designers)."""
    global _lib
    if _lib is None:
        path = path or os.environ.get("MSDR_LIB", LIB_PATH)
        if not os.path.exists(path):
            raise MsdrError(-100, "%s not built: run `make -C minimal-sdr_amd` (or __graft_entry__.build())" % path)
        _lib = C.CDLL(path)
        _lib.msdr_last_error.restype = C.c_char_p
        _lib.msdr_version.restype = C.c_char_p
        _lib.msdr_ctx_stream.restype = _p
        _lib.msdr_calc_FIR_coeffs.restype = None
        _lib.msdr_calc_FIR_coeffs.argtypes = [_p, C.c_int, C.c_float, C.c_float, C.c_int, C.c_float, C.c_float]
        _lib.msdr_calc_FIR_coeffs_pid.restype = None
        _lib.msdr_calc_FIR_coeffs_pid.argtypes = [_p, C.c_int, C.c_float, C.c_float, C.c_int, C.c_float, C.c_float]
        _lib.msdr_biquad_design.argtypes = [C.c_int, C.c_float, C.c_float, C.c_float, C.c_double, _p]
        _lib.msdr_biquad_df1_f32_cascade_info.argtypes = [C.c_uint8, _p, _p, _p, _p]
        _lib.msdr_biquad_df1_f32_state_to_cmsis.argtypes = [C.c_uint8, _p, _p, _p]
        _lib.msdr_biquad_df1_f32_state_from_cmsis.argtypes = [C.c_uint8, _p, _p, _p]
        _lib.msdr_biquad_df1_f32_set_coeffs.argtypes = [_p, _p]
        _lib.msdr_biquad_df1_f32_get_cmsis_state.argtypes = [_p, C.c_uint32, _p]
        _lib.msdr_fir_q15_set_coeffs.argtypes = [_p, _p]
        _lib.msdr_fir_f32_set_coeffs.argtypes = [_p, _p]
        _lib.msdr_chain_set_taps.argtypes = [_p, C.c_uint32, _p, _p]
        _lib.msdr_chain_set_osc.argtypes = [_p, _p, _p]
        _lib.msdr_chain_set_node_coefficients.argtypes = [_p, C.c_uint32, C.c_uint32, _p]
        # (looked up by name: a library built before these two calls existed -- MSDR_LIB pointing at an earlier build for an A/B timing --
        #  still loads, and a call of theirs on it raises AttributeError)
        for n, sig in (("msdr_chain_set_node_coefficients_channels", [_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _p]),
                       ("msdr_biquad_q15_set_coefficients_channels", [_p, C.c_uint32, C.c_uint32, C.c_uint32, _p]),
                       ("msdr_chain_set_taps_channels", [_p, C.c_uint32, C.c_uint32, _p, _p]),
                       ("msdr_fir_q15_set_coeffs_channels", [_p, C.c_uint32, C.c_uint32, _p]),
                       ("msdr_chain_set_taps_channels_f32", [_p, C.c_uint32, C.c_uint32, _p, _p]),
                       ("msdr_fir_f32_set_coeffs_channels", [_p, C.c_uint32, C.c_uint32, _p]),
                       ("msdr_chain_set_biquad_coeffs_channels", [_p, C.c_uint32, C.c_uint32, _p]),
                       ("msdr_biquad_df1_f32_set_coeffs_channels", [_p, C.c_uint32, C.c_uint32, _p]),
                       ("msdr_chain_set_osc_channels", [_p, C.c_uint32, C.c_uint32, _p, _p]),
                       ("msdr_chain_set_block_kernel", [_p, C.c_int]),
                       ("msdr_chain_set_block_kernel_q15", [_p, C.c_int]),
                       ("msdr_chain_set_input_rows", [_p, C.c_uint32, _p]),
                       ("msdr_chain_set_nco_channels", [_p, C.c_uint32, C.c_uint32, _p, _p]),
                       ("msdr_chain_get_nco", [_p, C.c_uint32, _p, _p]),
                       ("msdr_chain_set_decimation", [_p, C.c_uint32]),
                       ("msdr_chain_get_decimation", [_p, _p]),
                       ("msdr_chain_set_prefilter", [_p, C.c_uint32, C.c_uint32, _p]),
                       ("msdr_chain_set_prefilter_f32", [_p, C.c_uint32, C.c_uint32, _p]),
                       ("msdr_chain_get_prefilter", [_p, _p, _p]),
                       ("msdr_chain_get_geometry", [_p, _p]),
                       ("msdr_chain_get_iq_shared", [_p, _p]),
                       ("msdr_chain_set_meter", [_p, _p]),
                       ("msdr_chain_get_meter", [_p, _p]),
                       ("msdr_meter_dbfs", [C.c_double, C.c_uint64, C.c_double]),
                       ("msdr_chain_set_iq_out", [_p, _p, C.c_uint64]),
                       ("msdr_chain_get_iq_out", [_p, _p, _p]),
                       ("msdr_chain_set_complex_input", [_p, C.c_int, C.c_int]),
                       ("msdr_chain_get_complex_input", [_p, _p, _p]),
                       ("msdr_chain_set_gain", [_p, C.c_int]),
                       ("msdr_chain_get_gain", [_p, _p]),
                       ("msdr_chain_set_gain_channels", [_p, C.c_uint32, C.c_uint32, _p]),
                       ("msdr_chain_set_agc", [_p, _p, C.c_int32]),
                       ("msdr_chain_get_agc", [_p, C.c_uint32, _p]),
                       ("msdr_chain_set_bank_post", [_p, C.c_int]),
                       ("msdr_chain_get_bank_post", [_p, _p]),
                       ("msdr_chain_get_pll_state", [_p, C.c_uint32, _p]),
                       ("msdr_syncam_constants_rate", [C.c_double, _p]),
                       ("msdr_chain_set_pll_rate", [_p, C.c_double]),
                       ("msdr_chain_get_pll_rate", [_p, _p]),
                       ("msdr_chain_post_kernel", [_p]),
                       ("msdr_cfft64_q15", [_p, _p, C.c_uint64, _p, _p, C.c_uint32]),
                       ("msdr_cfft64_f32", [_p, _p, C.c_uint64, _p, _p, C.c_uint32]),
                       ("msdr_chain_set_spectrum", [_p, _p, _p, C.c_uint32]),
                       ("msdr_chain_get_spectrum", [_p, _p, _p, _p, _p]),
                       ("msdr_spectrum_dbfs", [C.c_double, C.c_double]),
                       ("msdr_nco_step", [C.c_double, C.c_double]),
                       ("msdr_nco_table", [_p]),
                       ("msdr_nco_q15", [_p, C.c_size_t, _p, _p]),
                       ("msdr_chain_get_fir_history", [_p, C.c_uint32, _p, C.c_uint32, _p]),
                       ("msdr_chain_get_cmsis_state", [_p, C.c_uint32, _p])):
            if hasattr(_lib, n):
                getattr(_lib, n).argtypes = sig
        if hasattr(_lib, "msdr_syncam_constants_rate"):
            _lib.msdr_syncam_constants_rate.restype = None
        if hasattr(_lib, "msdr_meter_dbfs"):
            _lib.msdr_meter_dbfs.restype = C.c_double
        if hasattr(_lib, "msdr_spectrum_dbfs"):
            _lib.msdr_spectrum_dbfs.restype = C.c_double
        if hasattr(_lib, "msdr_nco_step"):
            _lib.msdr_nco_step.restype = C.c_uint32
            _lib.msdr_nco_table.restype = None
            _lib.msdr_nco_q15.restype = None
        _lib.msdr_chain_set_biquad_coeffs.argtypes = [_p, _p]
        _lib.msdr_malloc.argtypes = [_p, C.c_size_t, _p]
        _lib.msdr_free.argtypes = [_p, _p]
        _lib.msdr_memcpy_h2d.argtypes = [_p, _p, _p, C.c_size_t]
        _lib.msdr_memcpy_d2h.argtypes = [_p, _p, _p, C.c_size_t]
        _lib.msdr_memset.argtypes = [_p, _p, C.c_int, C.c_size_t]
        _lib.msdr_ctx_create.argtypes = [C.c_int, _p, _p]
        _lib.msdr_chain_process.argtypes = [_p, _p, _p, C.c_uint64]
        _lib.msdr_chain_graph_create.argtypes = [_p, C.c_uint32, _p, _p, C.c_uint64, _p]
        _lib.msdr_chain_graph_launch.argtypes = [_p]
        _lib.msdr_chain_graph_destroy.argtypes = [_p]
        _lib.msdr_chain_get_kernel_time.argtypes = [_p, _p, _p, C.c_int]
        for n in ("msdr_fir_q15_process", "msdr_fir_f32_process", "msdr_biquad_df1_f32_process"):
            getattr(_lib, n).argtypes = [_p, _p, _p, C.c_uint32]
        _lib.msdr_biquad_q15_update.argtypes = [_p, _p, C.c_uint32]
        _lib.msdr_frontend_update.argtypes = [_p, _p, _p, C.c_uint32, C.c_uint32]
        _lib.msdr_frontend_prime.argtypes = [_p, _p, C.c_uint32]
        _lib.msdr_frontend_get_state.argtypes = [_p, C.c_uint32, _p]
        _lib.msdr_amp_q15.argtypes = [_p, C.c_int32, _p, C.c_uint32, C.c_uint32, _p]
        _lib.msdr_anr_q15.argtypes = [_p, _p, C.c_int32, _p, C.c_uint32]
        _lib.msdr_anr_get_state.argtypes = [_p, C.c_uint32, _p]
        _lib.msdr_chain_set_anr.argtypes = [_p, _p, C.c_int32]
        _lib.msdr_dac_format_q15.argtypes = [_p, _p, _p, C.c_uint32, C.c_uint32]
        _lib.msdr_syncam_q15.argtypes = [_p, _p, _p, _p, _p, C.c_uint32]
        _lib.msdr_syncam_get_state.argtypes = [_p, C.c_uint32, _p]
        _lib.msdr_syncam_constants.argtypes = [_p]
        _lib.msdr_syncam_constants.restype = None
        _lib.msdr_fir_f32_set_input_range.argtypes = [_p, C.c_float]
        _lib.msdr_rfft128_tables.argtypes = [_p]
        _lib.msdr_rfft128_tables.restype = None
        _lib.msdr_rfft_q15_init_check.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
        _lib.msdr_rfft128_q15.argtypes = [_p, _p, C.c_uint64, _p, _p, C.c_uint32]
        _lib.msdr_rfft128_q15_inplace.argtypes = [_p, _p, C.c_uint64, _p, _p, C.c_uint32]
        for n in ("msdr_mult_q15", "msdr_add_q15", "msdr_sub_q15"):
            getattr(_lib, n).argtypes = [_p, _p, C.c_uint64, _p, C.c_uint64, _p, C.c_uint32, C.c_uint32]
        _lib.msdr_copy_q15.argtypes = [_p, _p, C.c_uint64, _p, C.c_uint32, C.c_uint32]
        _lib.msdr_spectrum_create.argtypes = [_p, C.c_uint32, _p]
        _lib.msdr_spectrum_set_on.argtypes = [_p, C.c_int]
        _lib.msdr_spectrum_show.argtypes = [_p, _p, C.c_uint64, _p, _p, _p]
        _lib.msdr_spectrum_destroy.argtypes = [_p]
    return _lib


def _ck(rc):
    if rc != 0:
        raise MsdrError(rc, load_library().msdr_last_error().decode())


def _hp(a):
    return a.ctypes.data_as(_p) if a is not None else None


# ---- host-side designers (no device needed) ---------------------------------------------------
def calc_fir_coeffs(n, fc, astop=70.0, ftype=0, dfc=0.0, fs=24000.0, room=None, pi_double=False):
    """pi_double: `PI` as Arduino.h's double literal (what a Teensy build sees) instead of the vendored header's float."""
    buf = np.zeros(room or (2 * n + 8), np.int16)
    lib = load_library()
    f = lib.msdr_calc_FIR_coeffs_pid if pi_double else lib.msdr_calc_FIR_coeffs
    f(_hp(buf), int(n), float(fc), float(astop), int(ftype), float(dfc), float(fs))
    return buf


def biquad_design(kind, freq, q_or_gain, slope=1.0, fs=AUDIO_SAMPLE_RATE_EXACT):
    c = np.zeros(5, np.int32)
    _ck(load_library().msdr_biquad_design(int(kind), float(freq), float(q_or_gain), float(slope), float(fs), _hp(c)))
    return c


def biquad_cascade_info(coeffs):
    """(kappa, fp32_noise, cmsis_order) of a df1 cascade {b0,b1,b2,a1,a2} x stages -- host only."""
    c = np.ascontiguousarray(coeffs, np.float32).reshape(-1)
    k, nz, seq = C.c_double(0), C.c_double(0), C.c_int(0)
    _ck(load_library().msdr_biquad_df1_f32_cascade_info(C.c_uint8(c.size // 5), _hp(c) if c.size else None, C.byref(k), C.byref(nz), C.byref(seq)))
    return k.value, nz.value, bool(seq.value)


def biquad_state_to_cmsis(coeffs, lib_state):
    """The block-parallel kernels' 16-float state record -> arm_biquad_cascade_df1_f32's pState (4 per stage) -- host only."""
    c = np.ascontiguousarray(coeffs, np.float32).reshape(-1)
    st = np.ascontiguousarray(lib_state, np.float32).reshape(16)
    out = np.zeros(4 * (c.size // 5), np.float32)
    _ck(load_library().msdr_biquad_df1_f32_state_to_cmsis(C.c_uint8(c.size // 5), _hp(c), _hp(st), _hp(out)))
    return out


def biquad_state_from_cmsis(coeffs, pstate, d_hist=None):
    """pState -> the 16-float record (entries 0..7: the cascade's input history, taken from d_hist beyond the two newest)."""
    c = np.ascontiguousarray(coeffs, np.float32).reshape(-1)
    ps = np.ascontiguousarray(pstate, np.float32).reshape(-1)
    st = np.zeros(16, np.float32)
    if d_hist is not None:
        st[:len(d_hist)] = d_hist
    _ck(load_library().msdr_biquad_df1_f32_state_from_cmsis(C.c_uint8(c.size // 5), _hp(c), _hp(ps), _hp(st)))
    return st


class DeviceView:
    ptr = None


class DeviceArray:
    """A typed device buffer owned through msdr_malloc/msdr_free."""

    def __init__(self, ctx, shape, dtype):
        self.ctx, self.shape, self.dtype = ctx, tuple(np.atleast_1d(shape)), np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        ptr = _p()
        _ck(ctx.lib.msdr_malloc(ctx.h, self.nbytes, C.byref(ptr)))
        self.ptr = ptr.value
        ctx._adopt(self)

    def upload(self, a):
        a = np.ascontiguousarray(a, self.dtype)
        assert a.nbytes == self.nbytes, (a.shape, self.shape)
        _ck(self.ctx.lib.msdr_memcpy_h2d(self.ctx.h, self.ptr, _hp(a), self.nbytes))
        return self

    def download(self):
        out = np.empty(self.shape, self.dtype)
        _ck(self.ctx.lib.msdr_memcpy_d2h(self.ctx.h, _hp(out), self.ptr, self.nbytes))
        return out

    def offset(self, nbytes):
        """A non-owning view starting `nbytes` into this buffer (pointer arithmetic only)."""
        v = DeviceView()
        v.ptr = self.ptr + int(nbytes)
        return v

    def fill(self, byte):
        _ck(self.ctx.lib.msdr_memset(self.ctx.h, self.ptr, int(byte), self.nbytes))
        return self

    def free(self):
        if self.ptr:
            if getattr(self.ctx, "h", None):
                self.ctx.lib.msdr_free(self.ctx.h, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Context:
    def __init__(self, device=0, stream=None):
        self.lib = load_library()
        h = _p()
        _ck(self.lib.msdr_ctx_create(int(device), _p(stream) if stream else None, C.byref(h)))
        self.h = h

    def synchronize(self):
        _ck(self.lib.msdr_ctx_synchronize(self.h))

    def stream(self):
        """The hipStream_t the context enqueues on, as an int (0 = the NULL stream); e.g. msdr_dist.OverlappedGather(compute_stream=...)."""
        return int(self.lib.msdr_ctx_stream(self.h) or 0)

    def array(self, shape, dtype):
        return DeviceArray(self, shape, dtype)

    def to_device(self, a):
        a = np.ascontiguousarray(a)
        return DeviceArray(self, a.shape, a.dtype).upload(a)

    # ---- stateless stages -----------------------------------------------------------------------
    def enable_kernel_timing(self, on=True):
        """HIP events around the main kernel of the FIR stage mirrors (msdr_ctx_enable_kernel_timing)."""
        _ck(self.lib.msdr_ctx_enable_kernel_timing(self.h, int(on)))

    def kernel_time(self, reset=True):
        ms, n = C.c_double(0), C.c_uint64(0)
        _ck(self.lib.msdr_ctx_get_kernel_time(self.h, C.byref(ms), C.byref(n), int(reset)))
        return ms.value, n.value

    # the batched 64-point complex forward transform: transform f reads 64 pairs {I, Q} at d_pairs + f * stride_pairs pairs and writes
    # d_bins[f][64] pairs {re, im} (natural bin order) and / or d_power[f][64] (display order: column x = bin (x + 32) & 63); buffers are
    # DeviceArray / DeviceView / addresses, either output may be None
    def _cfft64(self, name, d_pairs, stride_pairs, nfft, d_bins, d_power):
        ptr = lambda b: None if b is None else int(getattr(b, "ptr", b))
        _ck(getattr(self.lib, name)(self.h, _p(ptr(d_pairs)), C.c_uint64(int(stride_pairs)), _p(ptr(d_bins)), _p(ptr(d_power)), C.c_uint32(int(nfft))))

    def cfft64_q15(self, d_pairs, stride_pairs, nfft, d_bins=None, d_power=None):
        """arm_cfft_q15 of length 64, forward, with bit reversal, bit-exact; power is the exact uint32 (msdr_cfft64_q15)"""
        self._cfft64("msdr_cfft64_q15", d_pairs, stride_pairs, nfft, d_bins, d_power)

    def cfft64_f32(self, d_pairs, stride_pairs, nfft, d_bins=None, d_power=None):
        """(1 / 64) sum_m z[m] exp(-2 pi i k m / 64) in fp32 (msdr_cfft64_f32)"""
        self._cfft64("msdr_cfft64_f32", d_pairs, stride_pairs, nfft, d_bins, d_power)

    def mix_fs4_q15(self, d_x, d_i, d_q, channels, n):
        _ck(self.lib.msdr_mix_fs4_q15(self.h, _p(d_x.ptr), _p(d_i.ptr), _p(d_q.ptr), C.c_uint32(channels), C.c_uint32(n)))

    def freqconv_q15(self, d_i, d_q, osc_i, osc_q, direction, passthrough, channels, n):
        oi, oq = np.ascontiguousarray(osc_i, np.int16), np.ascontiguousarray(osc_q, np.int16)
        _ck(self.lib.msdr_freqconv_q15(self.h, _p(d_i.ptr), _p(d_q.ptr), _hp(oi), _hp(oq), C.c_uint32(oi.size),
                                       int(direction), int(passthrough), C.c_uint32(channels), C.c_uint32(n)))

    # arm_mult_q15 / arm_add_q15 / arm_sub_q15 / arm_copy_q15 over a block batch: d_dst [channels][n] = op(a row c, b row c); a source's
    # row stride defaults to n (a dense batch), 0 = one row of n samples shared by every channel
    def _q15_binary(self, name, d_a, d_b, d_dst, channels, n, a_stride, b_stride):
        _ck(getattr(self.lib, name)(self.h, _p(d_a.ptr), C.c_uint64(n if a_stride is None else a_stride), _p(d_b.ptr),
                                    C.c_uint64(n if b_stride is None else b_stride), _p(d_dst.ptr), C.c_uint32(channels), C.c_uint32(n)))

    def mult_q15(self, d_a, d_b, d_dst, channels, n, a_stride=None, b_stride=None):
        self._q15_binary("msdr_mult_q15", d_a, d_b, d_dst, channels, n, a_stride, b_stride)

    def add_q15(self, d_a, d_b, d_dst, channels, n, a_stride=None, b_stride=None):
        self._q15_binary("msdr_add_q15", d_a, d_b, d_dst, channels, n, a_stride, b_stride)

    def sub_q15(self, d_a, d_b, d_dst, channels, n, a_stride=None, b_stride=None):
        self._q15_binary("msdr_sub_q15", d_a, d_b, d_dst, channels, n, a_stride, b_stride)

    def copy_q15(self, d_src, d_dst, channels, n, src_stride=None):
        _ck(self.lib.msdr_copy_q15(self.h, _p(d_src.ptr), C.c_uint64(n if src_stride is None else src_stride), _p(d_dst.ptr),
                                   C.c_uint32(channels), C.c_uint32(n)))

    def freqconv_f32(self, d_i, d_q, osc_i, osc_q, direction, passthrough, channels, n):
        oi, oq = np.ascontiguousarray(osc_i, np.float32), np.ascontiguousarray(osc_q, np.float32)
        _ck(self.lib.msdr_freqconv_f32(self.h, _p(d_i.ptr), _p(d_q.ptr), _hp(oi), _hp(oq), C.c_uint32(oi.size),
                                       int(direction), int(passthrough), C.c_uint32(channels), C.c_uint32(n)))

    def demod_q15(self, mode, d_i, d_q, d_out, channels, n, sqrt_kind=SQRT_F32, d_mode=None):
        _ck(self.lib.msdr_demod_q15(self.h, int(mode), _p(d_mode.ptr) if d_mode else None, int(sqrt_kind),
                                    _p(d_i.ptr), _p(d_q.ptr), _p(d_out.ptr), C.c_uint32(channels), C.c_uint32(n)))

    def demod_f32(self, mode, d_i, d_q, d_out, channels, n, d_mode=None):
        _ck(self.lib.msdr_demod_f32(self.h, int(mode), _p(d_mode.ptr) if d_mode else None,
                                    _p(d_i.ptr), _p(d_q.ptr), _p(d_out.ptr), C.c_uint32(channels), C.c_uint32(n)))

    def close(self):
        """Destroys the context.  Objects created on it that are still alive are released first: a handle must never reach
        the library after its context is gone (the garbage collector may run an object's __del__ long after the fixture that
        owned the context has closed it)."""
        if self.h:
            for obj in list(getattr(self, "_children", ())):
                try:
                    obj.close() if hasattr(obj, "close") else obj.free()
                except Exception:
                    pass
            self.lib.msdr_ctx_destroy(self.h)
            self.h = None

    def _adopt(self, obj):
        if not hasattr(self, "_children"):
            import weakref
            self._children = weakref.WeakSet()
        self._children.add(obj)


class _Instance:
    _destroy = None

    def __setattr__(self, name, value):
        object.__setattr__(self, name, value)
        if name == "ctx" and value is not None and hasattr(value, "_adopt"):
            value._adopt(self)

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None):            # context already destroyed: its objects went with it
                getattr(self.ctx.lib, self._destroy)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FirQ15(_Instance):
    """arm_fir_init_q15 / arm_fir_fast_q15, batched over channels."""
    _destroy = "msdr_fir_q15_destroy"

    def __init__(self, ctx, coeffs, channels):
        self.ctx = ctx
        c = np.ascontiguousarray(coeffs, np.int16)
        self.ntaps = int(c.size)
        h = _p()
        _ck(ctx.lib.msdr_fir_q15_create(ctx.h, C.c_uint16(c.size), _hp(c), C.c_uint32(channels), C.byref(h)))
        self.h = h

    def process(self, d_src, d_dst, n):
        _ck(self.ctx.lib.msdr_fir_q15_process(self.h, d_src.ptr, d_dst.ptr, n))

    def reset(self):
        _ck(self.ctx.lib.msdr_fir_q15_reset(self.h))

    def set_coeffs(self, coeffs):
        """pCoeffs rewritten under the running filter (UI.cpp:337-345): state kept."""
        c = np.ascontiguousarray(coeffs, np.int16)
        if c.size != self.ntaps:
            raise ValueError("set_coeffs: %d taps given, the instance has %d" % (c.size, self.ntaps))
        _ck(self.ctx.lib.msdr_fir_q15_set_coeffs(self.h, _hp(c)))

    def set_coeffs_channels(self, first_channel, coeffs):
        """pCoeffs of channel first_channel + i only := coeffs[i]: coeffs int16 [count, numTaps], CMSIS order; state kept."""
        c = _taps_per_channel("set_coeffs_channels", coeffs, self.ntaps)
        _ck(self.ctx.lib.msdr_fir_q15_set_coeffs_channels(self.h, C.c_uint32(first_channel), C.c_uint32(c.shape[0]), _hp(c)))


class FirF32(_Instance):
    """arm_fir_init_f32 / arm_fir_f32, batched over channels."""
    _destroy = "msdr_fir_f32_destroy"

    def __init__(self, ctx, coeffs, channels):
        self.ctx = ctx
        c = np.ascontiguousarray(coeffs, np.float32)
        self.ntaps = int(c.size)
        h = _p()
        _ck(ctx.lib.msdr_fir_f32_create(ctx.h, C.c_uint16(c.size), _hp(c), C.c_uint32(channels), C.byref(h)))
        self.h = h

    def process(self, d_src, d_dst, n):
        _ck(self.ctx.lib.msdr_fir_f32_process(self.h, d_src.ptr, d_dst.ptr, n))

    def reset(self):
        _ck(self.ctx.lib.msdr_fir_f32_reset(self.h))

    def set_coeffs(self, coeffs):
        c = np.ascontiguousarray(coeffs, np.float32)
        if c.size != self.ntaps:
            raise ValueError("set_coeffs: %d taps given, the instance has %d" % (c.size, self.ntaps))
        _ck(self.ctx.lib.msdr_fir_f32_set_coeffs(self.h, _hp(c)))

    def set_coeffs_channels(self, first_channel, coeffs):
        """pCoeffs of channel first_channel + i only := coeffs[i]: coeffs float32 [count, numTaps], CMSIS order; state kept."""
        c = _taps_per_channel("set_coeffs_channels", coeffs, self.ntaps, np.float32)
        _ck(self.ctx.lib.msdr_fir_f32_set_coeffs_channels(self.h, C.c_uint32(first_channel), C.c_uint32(c.shape[0]), _hp(c)))

    def set_input_range(self, max_abs):
        _ck(self.ctx.lib.msdr_fir_f32_set_input_range(self.h, C.c_float(max_abs)))

    def kernel_name(self):
        f = self.ctx.lib.msdr_fir_f32_kernel_name
        f.restype = C.c_char_p
        f.argtypes = [_p]
        return f(self.h).decode()


class BiquadDf1F32(_Instance):
    """arm_biquad_cascade_df1_init_f32 / arm_biquad_cascade_df1_f32, batched over channels."""
    _destroy = "msdr_biquad_df1_f32_destroy"

    def __init__(self, ctx, coeffs, channels):
        self.ctx = ctx
        c = np.ascontiguousarray(coeffs, np.float32).reshape(-1)
        self.stages = int(c.size // 5)
        h = _p()
        _ck(ctx.lib.msdr_biquad_df1_f32_create(ctx.h, C.c_uint8(c.size // 5), _hp(c) if c.size else None,
                                               C.c_uint32(channels), C.byref(h)))
        self.h = h

    def process(self, d_src, d_dst, n):
        _ck(self.ctx.lib.msdr_biquad_df1_f32_process(self.h, d_src.ptr, d_dst.ptr, n))

    def reset(self):
        _ck(self.ctx.lib.msdr_biquad_df1_f32_reset(self.h))

    def set_coeffs(self, coeffs):
        """pCoeffs rewritten under the running cascade: continues from CMSIS' pState."""
        c = np.ascontiguousarray(coeffs, np.float32).reshape(-1)
        if c.size != 5 * self.stages:
            raise ValueError("set_coeffs: %d values given, the cascade has %d stages x 5" % (c.size, self.stages))
        _ck(self.ctx.lib.msdr_biquad_df1_f32_set_coeffs(self.h, _hp(c)))

    def set_coeffs_channels(self, first_channel, coeffs):
        """pCoeffs of channel first_channel + i only := coeffs[i]: coeffs float32 [count, stages, 5] or [count, 5 * stages]; state kept (CMSIS order)."""
        c = _cascade_per_channel("set_coeffs_channels", coeffs, self.stages)
        _ck(self.ctx.lib.msdr_biquad_df1_f32_set_coeffs_channels(self.h, C.c_uint32(first_channel), C.c_uint32(c.shape[0]), _hp(c)))

    def cmsis_state(self, channel, stages):
        out = np.zeros(4 * stages, np.float32)
        _ck(self.ctx.lib.msdr_biquad_df1_f32_get_cmsis_state(self.h, C.c_uint32(channel), _hp(out)))
        return out


def _coefs_per_channel(what, coefs):
    c = np.ascontiguousarray(coefs, np.int32)
    if c.ndim != 2 or c.shape[1] != 5:
        raise ValueError("%s: one row of 5 words (b0, b1, b2, a1, a2) per channel, shape %s given" % (what, (c.shape,)))
    return c


def _cascade_per_channel(what, coeffs, stages):
    c = np.ascontiguousarray(coeffs, np.float32)
    if stages < 1 or not ((c.ndim == 3 and c.shape[1:] == (stages, 5)) or (c.ndim == 2 and c.shape[1] == 5 * stages)):
        raise ValueError("%s: one row of %d stages x 5 coefficients per channel (numStages is fixed at creation, as in CMSIS), shape %s given" % (what, stages, (c.shape,)))
    return c.reshape(c.shape[0], 5 * stages)


def _taps_per_channel(what, coeffs, ntaps, dtype=np.int16):
    c = np.ascontiguousarray(coeffs, dtype)
    if c.ndim != 2 or c.shape[1] != ntaps:
        raise ValueError("%s: one row of %d taps per channel (numTaps is fixed at creation, as in CMSIS), shape %s given" % (what, ntaps, (c.shape,)))
    return c


def _osc_per_channel(what, tab, osc_len, arith):
    t = np.asarray(tab)
    if arith == ARITH_Q15 and t.dtype.kind not in "iu":
        raise ValueError("%s: a Q15 chain takes integer tables (q15_t), dtype %s given" % (what, t.dtype))
    if arith == ARITH_F32 and t.dtype.kind not in "fiu":
        raise ValueError("%s: an fp32 chain takes real tables (float32_t), dtype %s given" % (what, t.dtype))
    if t.ndim != 2 or t.shape[1] != osc_len:
        raise ValueError("%s: one row of %d entries per channel (osc_len is fixed at creation), shape %s given" % (what, osc_len, (t.shape,)))
    if arith == ARITH_Q15 and t.size and (t.min() < -32768 or t.max() > 32767):
        raise ValueError("%s: a table entry outside int16" % what)
    return np.ascontiguousarray(t, np.float32 if arith == ARITH_F32 else np.int16)


def _input_rows(what, rows, channels, n_inputs):
    r = np.asarray(rows)
    if r.dtype.kind not in "iu":
        raise ValueError("%s: row indices are integers, dtype %s given" % (what, r.dtype))
    if r.ndim != 1 or r.shape[0] != channels:
        raise ValueError("%s: one row index per channel (%d), shape %s given" % (what, channels, (r.shape,)))
    if r.size and r.min() < 0:
        raise ValueError("%s: a negative row index" % what)
    if n_inputs is None:
        n_inputs = int(r.max()) + 1 if r.size else 0
    if isinstance(n_inputs, bool) or not isinstance(n_inputs, (int, np.integer)) or n_inputs <= 0 or n_inputs > 0x7fffffff:
        raise ValueError("%s: n_inputs is a positive row count, %r given" % (what, n_inputs))
    if r.size and r.max() >= n_inputs:
        raise ValueError("%s: row index %d, but the input has %d rows" % (what, int(r.max()), n_inputs))
    return np.ascontiguousarray(r, np.uint32), int(n_inputs)


def _nco_words(what, a, count):
    """a one-dimensional array of uint32 words (steps, phases); count: the length it must have, or None"""
    t = np.asarray(a)
    if t.dtype.kind not in "iu":
        raise ValueError("%s: steps and phases are unsigned 32-bit integers, dtype %s given" % (what, t.dtype))
    if t.ndim != 1 or t.size == 0:
        raise ValueError("%s: one word per channel, shape %s given" % (what, (t.shape,)))
    if count is not None and t.size != count:
        raise ValueError("%s: %d phases for %d steps" % (what, t.size, count))
    if t.min() < 0 or t.max() > 0xFFFFFFFF:
        raise ValueError("%s: a word outside uint32" % what)
    return np.ascontiguousarray(t, np.uint32)


def spectrum_dbfs(power, full_scale=32768.0):
    """msdr_spectrum_dbfs: 10 log10(power / (full_scale^2 / 4)) -- an entry of Chain.set_spectrum()'s power rows in dB relative to a full-scale
    real carrier on a bin centre behind a unity-gain channel filter; -inf for power <= 0.  full_scale: 32768 for Q15, 32768 * in_scale for F32."""
    return float(load_library().msdr_spectrum_dbfs(float(power), float(full_scale)))


def meter_dbfs(sum_sq, n_out, full_scale=32768.0):
    """msdr_meter_dbfs: 10 log10((sum_sq / n_out) / (full_scale^2 / 4)) -- a Chain.set_meter() entry over n_out outputs in dB relative to a
    full-scale carrier at the tuned frequency (full_scale = 32768 for Q15, 32768 * in_scale for F32); -inf for sum_sq <= 0 or n_out == 0.
    Host only."""
    return float(load_library().msdr_meter_dbfs(float(sum_sq), int(n_out), float(full_scale)))


def nco_step(f_hz, fs_hz=24000.0):
    """msdr_nco_step: llround(f / fs * 2^32) mod 2^32 -- the step of a phase-accumulator oscillator at f_hz (negative wraps).  Host only."""
    return int(load_library().msdr_nco_step(float(f_hz), float(fs_hz)))


def nco_table():
    """msdr_nco_table: the 1025-entry sine table T[i] = lround(32767 sin(2 pi i / 1024)) the oscillator interpolates in.  Host only."""
    t = np.zeros(1025, np.int16)
    load_library().msdr_nco_table(_hp(t))
    return t


def nco_q15(phases):
    """msdr_nco_q15: (sin, cos) as int16 arrays for uint32 phases, exactly what the kernels compute.  Host only."""
    ph = np.ascontiguousarray(_nco_words("nco_q15", np.asarray(phases).reshape(-1), None))
    s, c = np.zeros(ph.size, np.int16), np.zeros(ph.size, np.int16)
    load_library().msdr_nco_q15(_hp(ph), C.c_size_t(ph.size), _hp(s), _hp(c))
    return s, c


def _kernel_name(f, h):
    f.restype = C.c_char_p
    f.argtypes = [_p]
    return f(h).decode()


class BiquadQ15(_Instance):
    """AudioFilterBiquad: setCoefficients(stage, coef[5]) / update(), batched over channels."""
    _destroy = "msdr_biquad_q15_destroy"

    def __init__(self, ctx, channels):
        self.ctx = ctx
        h = _p()
        _ck(ctx.lib.msdr_biquad_q15_create(ctx.h, C.c_uint32(channels), C.byref(h)))
        self.h = h

    def set_coefficients(self, stage, coef):
        c = np.ascontiguousarray(coef, np.int32)
        _ck(self.ctx.lib.msdr_biquad_q15_set_coefficients(self.h, C.c_uint32(stage), _hp(c)))

    def set_coefficients_channels(self, first_channel, stage, coefs):
        """setCoefficients(stage, coefs[i]) on channel first_channel + i only: coefs int32 [count, 5]."""
        c = _coefs_per_channel("set_coefficients_channels", coefs)
        _ck(self.ctx.lib.msdr_biquad_q15_set_coefficients_channels(self.h, C.c_uint32(first_channel), C.c_uint32(c.shape[0]), C.c_uint32(stage), _hp(c)))

    def update(self, d_data, n):
        _ck(self.ctx.lib.msdr_biquad_q15_update(self.h, d_data.ptr, n))

    def last_kernel(self):
        """msdr_biquad_q15_last_kernel: the kernel the last update() launched, with its template arguments ("" before the first)."""
        return _kernel_name(self.ctx.lib.msdr_biquad_q15_last_kernel, self.h)

    def definition(self, channel=0):
        d = np.zeros(32, np.int32)
        _ck(self.ctx.lib.msdr_biquad_q15_get_definition(self.h, C.c_uint32(channel), _hp(d)))
        return d


class Frontend(_Instance):
    """adc1's DC block + amp_adc + AGC(), batched over channels; state per channel as the sketch's statics."""
    _destroy = "msdr_frontend_destroy"

    def __init__(self, ctx, channels):
        self.ctx = ctx
        h = _p()
        _ck(ctx.lib.msdr_frontend_create(ctx.h, C.c_uint32(channels), C.byref(h)))
        self.h = h

    def prime(self, first_conversion):
        v = np.ascontiguousarray(np.atleast_1d(first_conversion), np.uint16)
        _ck(self.ctx.lib.msdr_frontend_prime(self.h, _hp(v), C.c_uint32(v.size)))

    def set_agc(self, on):
        _ck(self.ctx.lib.msdr_frontend_set_agc(self.h, int(bool(on))))

    def gain(self, n):
        _ck(self.ctx.lib.msdr_frontend_gain(self.h, C.c_float(n)))

    def update(self, d_adc, d_out, n, stages=FE_ALL):
        _ck(self.ctx.lib.msdr_frontend_update(self.h, d_adc.ptr if hasattr(d_adc, "ptr") else d_adc,
                                              d_out.ptr if hasattr(d_out, "ptr") else d_out, C.c_uint32(n), C.c_uint32(stages)))

    def last_kernel(self):
        """msdr_frontend_last_kernel: the kernel the last update() launched, with its template arguments ("" before the first)."""
        return _kernel_name(self.ctx.lib.msdr_frontend_last_kernel, self.h)

    def state(self, channel=0):
        st = np.zeros(32, np.int32)
        _ck(self.ctx.lib.msdr_frontend_get_state(self.h, C.c_uint32(channel), _hp(st)))
        return st


class Syncam(_Instance):
    """The PLL branch of the demod switch (Minimal-SDR.ino:631-688), batched over channels."""
    _destroy = "msdr_syncam_destroy"

    def __init__(self, ctx, channels):
        self.ctx = ctx
        h = _p()
        _ck(ctx.lib.msdr_syncam_create(ctx.h, C.c_uint32(channels), C.byref(h)))
        self.h = h

    def process(self, d_i, d_q, d_out, n, d_mode=None):
        _ck(self.ctx.lib.msdr_syncam_q15(self.h, d_mode.ptr if d_mode is not None else None, d_i.ptr, d_q.ptr, d_out.ptr, C.c_uint32(n)))

    def reset(self):
        _ck(self.ctx.lib.msdr_syncam_reset(self.h))

    def state(self, channel=0):
        st = np.zeros(3, np.float32)
        _ck(self.ctx.lib.msdr_syncam_get_state(self.h, C.c_uint32(channel), _hp(st)))
        return st


class Anr(_Instance):
    """LMS automatic notch / noise reduction (Minimal-SDR.ino:702-770), batched over channels."""
    _destroy = "msdr_anr_destroy"

    def __init__(self, ctx, channels):
        self.ctx = ctx
        h = _p()
        _ck(ctx.lib.msdr_anr_create(ctx.h, C.c_uint32(channels), C.byref(h)))
        self.h = h

    def process(self, d_data, n, anr_on=1, d_anr_on=None):
        _ck(self.ctx.lib.msdr_anr_q15(self.h, d_anr_on.ptr if d_anr_on is not None else None, C.c_int32(anr_on), d_data.ptr, C.c_uint32(n)))

    def reset(self):
        _ck(self.ctx.lib.msdr_anr_reset(self.h))

    def state(self, channel=0):
        st = np.zeros(196, np.float32)
        _ck(self.ctx.lib.msdr_anr_get_state(self.h, C.c_uint32(channel), _hp(st)))
        return st


def dac_format_q15(ctx, d_src, d_dest, channels, n):
    _ck(ctx.lib.msdr_dac_format_q15(ctx.h, d_src.ptr if d_src is not None else None, d_dest.ptr, C.c_uint32(channels), C.c_uint32(n)))


def rfft128_tables():
    """(twiddleCoef_64_q15[96], realCoefAQ15[::64 pairs][128], realCoefBQ15[::64 pairs][128]) -- host side."""
    t = np.zeros(352, np.int16)
    load_library().msdr_rfft128_tables(_hp(t))
    return t[:96], t[96:224], t[224:]


def rfft128_q15(ctx, d_src, src_stride, nfft, d_fft_out=None, d_columns=None):
    """arm_rfft_q15(&FFT(128, 0, 1), ...) batched (UI.cpp:551) + showSpectrum's column heights (UI.cpp:557-572)."""
    _ck(ctx.lib.msdr_rfft128_q15(ctx.h, d_src.ptr, C.c_uint64(src_stride), d_fft_out.ptr if d_fft_out is not None else None,
                                 d_columns.ptr if d_columns is not None else None, C.c_uint32(nfft)))


def rfft128_q15_inplace(ctx, d_src, src_stride, nfft, d_fft_out=None, d_columns=None):
    """rfft128_q15, and like arm_rfft_q15 (arm_rfft_q15.c:103-107) each transform's 128 samples of d_src are overwritten with the CMSIS
    work buffer (the complex FFT's output after the bit reversal)."""
    _ck(ctx.lib.msdr_rfft128_q15_inplace(ctx.h, d_src.ptr, C.c_uint64(src_stride), d_fft_out.ptr if d_fft_out is not None else None,
                                         d_columns.ptr if d_columns is not None else None, C.c_uint32(nfft)))


class Spectrum(_Instance):
    """initSpectrum() / showSpectrum() (UI.cpp:520-592): Spectrum_on + the every-25th-call cadence."""
    _destroy = "msdr_spectrum_destroy"

    def __init__(self, ctx, channels):
        self.ctx = ctx
        h = _p()
        _ck(ctx.lib.msdr_spectrum_create(ctx.h, C.c_uint32(channels), C.byref(h)))
        self.h = h

    def set_on(self, on):
        _ck(self.ctx.lib.msdr_spectrum_set_on(self.h, int(on)))

    def show(self, d_data, channel_stride, d_fft_out=None, d_columns=None):
        drawn = C.c_int(0)
        _ck(self.ctx.lib.msdr_spectrum_show(self.h, d_data.ptr, C.c_uint64(channel_stride),
                                            d_fft_out.ptr if d_fft_out is not None else None,
                                            d_columns.ptr if d_columns is not None else None, C.byref(drawn)))
        return bool(drawn.value)


def syncam_constants():
    c = np.zeros(4, np.float32)
    load_library().msdr_syncam_constants(_hp(c))
    return c


def syncam_constants_rate(sample_rate):
    """omega_min, omega_max, g1, g2 of the PLL evaluated for `sample_rate` (msdr_syncam_constants_rate): syncam_constants() at 24000, bit for
    bit; what Chain.set_pll_rate puts in force for a bank that runs its loop at fs / D"""
    c = np.zeros(4, np.float32)
    load_library().msdr_syncam_constants_rate(C.c_double(float(sample_rate)), _hp(c))
    return c


def amp_multiplier(n):
    lib = load_library()
    lib.msdr_amp_multiplier.restype = C.c_int32
    lib.msdr_amp_multiplier.argtypes = [C.c_float]
    return int(lib.msdr_amp_multiplier(C.c_float(n)))


def amp_q15(ctx, multiplier, d_data, channels, n):
    t = C.c_int(0)
    _ck(ctx.lib.msdr_amp_q15(ctx.h, C.c_int32(multiplier), d_data.ptr, C.c_uint32(channels), C.c_uint32(n), C.byref(t)))
    return bool(t.value)


class ChainGraph:
    """`ticks` consecutive block-cadence calls of one chain as ONE HIP graph (include/msdr.h: msdr_chain_graph_*)."""

    def __init__(self, chain, d_ifs, d_audios, n):
        assert len(d_ifs) == len(d_audios)
        self.chain, self.ticks = chain, len(d_ifs)
        pi = (C.c_void_p * self.ticks)(*[(d.ptr if hasattr(d, "ptr") else int(d)) for d in d_ifs])
        po = (C.c_void_p * self.ticks)(*[(d.ptr if hasattr(d, "ptr") else int(d)) for d in d_audios])
        self.h = C.c_void_p()
        _ck(chain.ctx.lib.msdr_chain_graph_create(chain.h, self.ticks, pi, po, n, C.byref(self.h)))

    def launch(self):
        _ck(self.chain.ctx.lib.msdr_chain_graph_launch(self.h))

    def close(self):
        if self.h:
            self.chain.ctx.lib.msdr_chain_graph_destroy(self.h)
            self.h = None


class Chain(_Instance):
    """The fused chain (msdr_chain_*): demodulation() + the biquad nodes behind it."""
    _destroy = "msdr_chain_destroy"

    def __init__(self, ctx, arith, channels, coeffs_i, coeffs_q, mixer=MIXER_FS4, mode=MODE_AM, modes=None,
                 tapsets=None, osc_i=None, osc_q=None, sqrt_kind=SQRT_F32, in_scale=0.0, biquad_coeffs=None,
                 biquad_nodes=(), time_segments=0, biquad_warmup=0, flags=0):
        self.ctx, self.arith, self.channels = ctx, arith, channels
        tdt = np.float32 if arith == ARITH_F32 else np.int16
        ci = [np.ascontiguousarray(c, tdt) for c in (coeffs_i if isinstance(coeffs_i, (list, tuple)) else [coeffs_i])]
        cq = [np.ascontiguousarray(c, tdt) for c in (coeffs_q if isinstance(coeffs_q, (list, tuple)) else [coeffs_q])]
        keep = [ci, cq]
        cfg = ChainConfig()
        cfg.struct_size = C.sizeof(ChainConfig)
        cfg.arith, cfg.channels, cfg.mixer = arith, channels, mixer
        cfg.num_taps, cfg.num_tapsets = ci[0].size, len(ci)
        self.ntaps, self.osc_len, self.stages = int(ci[0].size), 0, 0     # what the setters' arrays must hold (the C side copies that many elements)
        for k in range(len(ci)):
            cfg.coeffs_i[k], cfg.coeffs_q[k] = _hp(ci[k]), _hp(cq[k])
        cfg.default_mode = mode
        if modes is not None:
            m = np.ascontiguousarray(modes, np.int32)
            keep.append(m)
            cfg.mode = _hp(m)
        if tapsets is not None:
            t = np.ascontiguousarray(tapsets, np.int32)
            keep.append(t)
            cfg.tapset = _hp(t)
        cfg.sqrt_kind = sqrt_kind
        if osc_i is not None:
            oi, oq = np.ascontiguousarray(osc_i, tdt), np.ascontiguousarray(osc_q, tdt)
            keep += [oi, oq]
            cfg.osc_len, cfg.osc_i, cfg.osc_q = oi.size, _hp(oi), _hp(oq)
            self.osc_len = int(oi.size)
        cfg.in_scale = in_scale
        if biquad_coeffs is not None and arith == ARITH_F32:
            b = np.ascontiguousarray(biquad_coeffs, np.float32).reshape(-1)
            keep.append(b)
            cfg.num_biquad_stages, cfg.biquad_coeffs = b.size // 5, _hp(b)
            self.stages = int(b.size // 5)
        if arith == ARITH_Q15:
            cfg.num_biquad_nodes = len(biquad_nodes)
            for k, stages in enumerate(biquad_nodes):
                s = np.ascontiguousarray(stages, np.int32).reshape(-1)
                keep.append(s)
                cfg.node_stages[k], cfg.node_coefs[k] = s.size // 5, _hp(s)
        cfg.time_segments, cfg.biquad_warmup, cfg.flags = time_segments, biquad_warmup, flags
        h = _p()
        _ck(ctx.lib.msdr_chain_create(ctx.h, C.byref(cfg), C.byref(h)))
        self.h = h

    def process(self, d_if, d_audio, n):
        """d_if / d_audio: DeviceArray or raw device pointers (int).  d_audio None: an I/Q-only call (accepted while set_iq_out() has a buffer)."""
        pi = d_if.ptr if hasattr(d_if, "ptr") else int(d_if)
        po = None if d_audio is None else d_audio.ptr if hasattr(d_audio, "ptr") else int(d_audio)
        _ck(self.ctx.lib.msdr_chain_process(self.h, pi, po, n))

    def graph(self, d_ifs, d_audios, n):
        """msdr_chain_graph_create: len(d_ifs) (even) consecutive calls of n samples as one HIP graph; .launch() enqueues them."""
        return ChainGraph(self, d_ifs, d_audios, n)

    def reset(self):
        _ck(self.ctx.lib.msdr_chain_reset(self.h))

    def init_fir(self):
        """init_FIR() (Minimal-SDR.ino:901-930): FIR state only."""
        _ck(self.ctx.lib.msdr_chain_init_fir(self.h))

    def set_mode(self, channel, mode, tapset=0):
        _ck(self.ctx.lib.msdr_chain_set_mode(self.h, C.c_uint32(channel), C.c_int32(mode), C.c_int32(tapset)))

    def set_anr(self, anr_on=None, anr_on_all=0):
        a = np.ascontiguousarray(anr_on, np.int32) if anr_on is not None else None
        _ck(self.ctx.lib.msdr_chain_set_anr(self.h, _hp(a), C.c_int32(anr_on_all)))

    # ---- live updates, every filter state kept (include/msdr.h) ----
    def set_taps(self, tapset, coeffs_i, coeffs_q):
        tdt = np.float32 if self.arith == ARITH_F32 else np.int16
        ci, cq = np.ascontiguousarray(coeffs_i, tdt), np.ascontiguousarray(coeffs_q, tdt)
        if ci.size != self.ntaps or cq.size != self.ntaps:
            raise ValueError("set_taps: %d / %d taps given, the chain was created with %d (numTaps is fixed at creation, as in CMSIS)" % (ci.size, cq.size, self.ntaps))
        _ck(self.ctx.lib.msdr_chain_set_taps(self.h, C.c_uint32(tapset), _hp(ci), _hp(cq)))

    def set_taps_channels(self, first_channel, coeffs_i, coeffs_q=None):
        """Q15: channel first_channel + i gets FIR coefficients of its own, coeffs_i[i] / coeffs_q[i] (int16 [count, numTaps], CMSIS order);
        coeffs_q = None: the same array behind both filters (init_FIR() for AM / SYNCAM).  Every state kept."""
        ci = _taps_per_channel("set_taps_channels", coeffs_i, self.ntaps)
        cq = None if coeffs_q is None else _taps_per_channel("set_taps_channels", coeffs_q, self.ntaps)
        if cq is not None and cq.shape != ci.shape:
            raise ValueError("set_taps_channels: coeffs_i %s and coeffs_q %s differ in shape" % ((ci.shape,), (cq.shape,)))
        _ck(self.ctx.lib.msdr_chain_set_taps_channels(self.h, C.c_uint32(first_channel), C.c_uint32(ci.shape[0]), _hp(ci), _hp(cq)))

    def set_taps_channels_f32(self, first_channel, coeffs_i, coeffs_q=None):
        """F32: channel first_channel + i gets FIR coefficients of its own, coeffs_i[i] / coeffs_q[i] (float32 [count, numTaps], CMSIS order);
        coeffs_q = None: the same array behind both filters.  Every state kept; chain_f32pc_kernel from the first call on."""
        ci = _taps_per_channel("set_taps_channels_f32", coeffs_i, self.ntaps, np.float32)
        cq = None if coeffs_q is None else _taps_per_channel("set_taps_channels_f32", coeffs_q, self.ntaps, np.float32)
        if cq is not None and cq.shape != ci.shape:
            raise ValueError("set_taps_channels_f32: coeffs_i %s and coeffs_q %s differ in shape" % ((ci.shape,), (cq.shape,)))
        _ck(self.ctx.lib.msdr_chain_set_taps_channels_f32(self.h, C.c_uint32(first_channel), C.c_uint32(ci.shape[0]), _hp(ci), _hp(cq)))

    def set_osc(self, osc_i, osc_q):
        tdt = np.float32 if self.arith == ARITH_F32 else np.int16
        oi, oq = np.ascontiguousarray(osc_i, tdt), np.ascontiguousarray(osc_q, tdt)
        if self.osc_len and (oi.size != self.osc_len or oq.size != self.osc_len):
            raise ValueError("set_osc: tables of %d / %d entries, the chain's have %d" % (oi.size, oq.size, self.osc_len))
        _ck(self.ctx.lib.msdr_chain_set_osc(self.h, _hp(oi), _hp(oq)))

    def set_osc_channels(self, first_channel, osc_i, osc_q):
        """channel first_channel + i gets oscillator tables of its own, osc_i[i] / osc_q[i] ([count, osc_len]; int16 on a Q15 chain, float32 on
        an fp32 chain): tune() of ONE receiver.  The table position carries on, every state kept; chain_q15pco_kernel / chain_f32pco_kernel
        from the first call on."""
        oi = _osc_per_channel("set_osc_channels", osc_i, self.osc_len, self.arith)
        oq = _osc_per_channel("set_osc_channels", osc_q, self.osc_len, self.arith)
        if oi.shape != oq.shape:
            raise ValueError("set_osc_channels: osc_i %s and osc_q %s differ in shape" % ((oi.shape,), (oq.shape,)))
        _ck(self.ctx.lib.msdr_chain_set_osc_channels(self.h, C.c_uint32(first_channel), C.c_uint32(oi.shape[0]), _hp(oi), _hp(oq)))

    def set_nco_channels(self, first_channel, steps, phases=None):
        """channel first_channel + i gets a phase-accumulator oscillator with step steps[i] (uint32 [count]; nco_step(f, fs)) from its next
        sample on: tune() of ONE receiver to ANY frequency.  phases = None: the phase carries on (a phase-continuous retune); otherwise the next
        sample has phase phases[i] (uint32 [count]).  Every state kept; chain_q15pcn_kernel / chain_f32pcn_kernel from the first call on, which
        names every channel over a clear history."""
        st = _nco_words("set_nco_channels", steps, None)
        ph = None if phases is None else _nco_words("set_nco_channels", phases, st.size)
        _ck(self.ctx.lib.msdr_chain_set_nco_channels(self.h, C.c_uint32(first_channel), C.c_uint32(st.size), _hp(st), _hp(ph)))

    def nco(self, channel):
        """(step, phase of the NEXT sample) of `channel`'s phase-accumulator oscillator (msdr_chain_get_nco)"""
        st, ph = C.c_uint32(0), C.c_uint32(0)
        _ck(self.ctx.lib.msdr_chain_get_nco(self.h, C.c_uint32(channel), C.byref(st), C.byref(ph)))
        return st.value, ph.value

    def set_decimation(self, D):
        """a chain in phase-accumulator mode becomes a bank of digital down-converters: output m of a call is the demodulator's value at input
        sample m * D + D - 1, d_audio is [channels, n // D] and the nodes / the cascade behind the kernel run at fs / D.  1 = off; every state
        kept (msdr_chain_set_decimation)."""
        _ck(self.ctx.lib.msdr_chain_set_decimation(self.h, C.c_uint32(D)))

    def decimation(self):
        """the decimation in force (msdr_chain_get_decimation)"""
        d = C.c_uint32(0)
        _ck(self.ctx.lib.msdr_chain_get_decimation(self.h, C.byref(d)))
        return d.value

    def set_prefilter(self, D1, taps):
        """two-stage decimation: ONE real row `taps` in CMSIS order (int16 on Q15 chains, even count; float32 on F32), the same for the I and
        the Q stream of every receiver, decimates the mixed stream by D1 (2, 4, 8, 16 or 32) in front of the channel pair, which runs at
        fs / D1 and decimates by set_decimation's factor; d_audio is [channels, n // (D1 * D)].  Over a clear history only (before the first
        process(), or directly after reset() / init_fir()); D1 = 1 or no taps: off (msdr_chain_set_prefilter / _f32)."""
        f32 = self.arith == ARITH_F32
        t = np.ascontiguousarray(np.zeros(0) if taps is None else taps, np.float32 if f32 else np.int16).ravel()
        fn = self.ctx.lib.msdr_chain_set_prefilter_f32 if f32 else self.ctx.lib.msdr_chain_set_prefilter
        _ck(fn(self.h, C.c_uint32(D1), C.c_uint32(t.size), _hp(t) if t.size else None))

    def prefilter(self):
        """(D1, num_taps) of the prefilter in force, (1, 0) while off (msdr_chain_get_prefilter)"""
        d, n = C.c_uint32(0), C.c_uint32(0)
        _ck(self.ctx.lib.msdr_chain_get_prefilter(self.h, C.byref(d), C.byref(n)))
        return d.value, n.value

    def set_meter(self, d_meter):
        """The S-meter: from the next process() on every call overwrites d_meter[channels] -- a device buffer of 8-byte entries (DeviceArray /
        DeviceView / address), uint64 for Q15 chains, float64 for F32 -- with each channel's sum of I^2 + Q^2 behind the channel filter over
        the call's outputs, stream-ordered.  None switches it off.  The per-channel kernel family from the first call on; every state kept
        (msdr_chain_set_meter)."""
        ptr = None if d_meter is None else int(getattr(d_meter, "ptr", d_meter))
        _ck(self.ctx.lib.msdr_chain_set_meter(self.h, _p(ptr)))
        self._meter = d_meter          # (the buffer stays the caller's; this keeps a DeviceArray alive while the kernels write it)

    def meter(self):
        """the address of the meter buffer in force, None on a chain without one (msdr_chain_get_meter)"""
        p = _p()
        _ck(self.ctx.lib.msdr_chain_get_meter(self.h, C.byref(p)))
        return p.value

    def set_spectrum(self, d_bins, d_power, every=0):
        """A panadapter line per receiver: while on, every process() keeps each receiver's most recent 64 pairs behind its channel filter (at
        fs / D) and, on showSpectrum's cadence (the first call, then every `every`-th; 0 = 25), overwrites d_bins[channels][64] pairs
        {re, im} (int16 / float32, natural bin order) and / or d_power[channels][64] (uint32 / float32, column 32 = the tuned frequency) with
        their 64-point transform -- 16-byte aligned device buffers (DeviceArray / DeviceView / address); one None: only the other is written,
        both None: off.  Chains with set_nco_channels only (msdr_chain_set_spectrum)."""
        ptr = lambda b: None if b is None else int(getattr(b, "ptr", b))
        _ck(self.ctx.lib.msdr_chain_set_spectrum(self.h, _p(ptr(d_bins)), _p(ptr(d_power)), C.c_uint32(int(every))))
        self._spectrum = (d_bins, d_power)          # (the buffers stay the caller's; this keeps DeviceArrays alive while the kernel writes them)

    def spectrum(self):
        """(address of the bins buffer or None, address of the power buffer or None, every, spectra drawn since the switch went on)
        (msdr_chain_get_spectrum)"""
        b, p, every, drawn = _p(), _p(), C.c_uint32(0), C.c_uint64(0)
        _ck(self.ctx.lib.msdr_chain_get_spectrum(self.h, C.byref(b), C.byref(p), C.byref(every), C.byref(drawn)))
        return b.value, p.value, every.value, drawn.value

    def set_iq_out(self, d_iq, pitch=0):
        """Baseband I/Q output: from the next process() on every call overwrites pairs 0 .. n_out - 1 of every row of d_iq[channels][pitch] -- a
        16-byte aligned device buffer (DeviceArray / DeviceView / address) of interleaved pairs {I, Q}, two int16 for Q15 chains, two float32
        for F32, pitch a non-zero multiple of 8 -- with the two FIR outputs behind each channel's filter, stream-ordered.  None switches it
        off.  While it is set process(d_if, None, n) is an I/Q-only call.  Chains with set_nco_channels only (msdr_chain_set_iq_out)."""
        ptr = None if d_iq is None else int(getattr(d_iq, "ptr", d_iq))
        _ck(self.ctx.lib.msdr_chain_set_iq_out(self.h, _p(ptr), C.c_uint64(int(pitch))))
        self._iq_out = d_iq          # (the buffer stays the caller's; this keeps a DeviceArray alive while the kernels write it)

    def iq_out(self):
        """(the address of the I/Q buffer in force or None, its pitch in pairs) (msdr_chain_get_iq_out)"""
        p, pitch = _p(), C.c_uint64()
        _ck(self.ctx.lib.msdr_chain_get_iq_out(self.h, C.byref(p), C.byref(pitch)))
        return p.value, pitch.value

    def set_complex_input(self, on, dir=0):
        """Complex I/Q input: from the next process() on d_if is [channels or n_inputs, n] PAIRS {I, Q} of two int16 (an int16 array
        [rows, n, 2], 4-byte aligned) and the kernels apply freq_conv's full mix in direction dir (0: down by the receiver's frequency, 1: up;
        Q = 0 with dir = 1 is the real chain).  Chains with set_nco_channels only, and only over a clear FIR history: before the first
        process(), or directly after reset() / init_fir() (msdr_chain_set_complex_input)."""
        _ck(self.ctx.lib.msdr_chain_set_complex_input(self.h, C.c_int(1 if on else 0), C.c_int(int(dir))))

    def complex_input(self):
        """(on, dir) in force (msdr_chain_get_complex_input)"""
        on, d = C.c_int(0), C.c_int(0)
        _ck(self.ctx.lib.msdr_chain_get_complex_input(self.h, C.byref(on), C.byref(d)))
        return bool(on.value), d.value

    def set_gain(self, on):
        """Per-receiver gain: while on, the pair behind every receiver's channel filter is multiplied by that receiver's gain on the FIR
        accumulators (Q15: ssat16((acc * multiplier) >> 31); F32: acc * gain) before demodulator, PLL hand-over and I/Q output see it -- the
        meter keeps the ungained pair -- and AGC() steps once behind every process().  On alone changes no output bit (gain 1.0, AGC off).
        Chains with set_nco_channels only (msdr_chain_set_gain)."""
        _ck(self.ctx.lib.msdr_chain_set_gain(self.h, C.c_int(1 if on else 0)))

    def gain(self):
        """whether gain is on (msdr_chain_get_gain)"""
        on = C.c_int(0)
        _ck(self.ctx.lib.msdr_chain_get_gain(self.h, C.byref(on)))
        return bool(on.value)

    def set_gain_channels(self, first_channel, gains):
        """receiver first_channel + i gets AGC_val = gains[i] (float32 [count]) and its multiplier from the next process() on: amp_adc.gain()
        of ONE receiver.  The AGC's ring is untouched (msdr_chain_set_gain_channels)."""
        g = np.ascontiguousarray(gains, np.float32).reshape(-1)
        _ck(self.ctx.lib.msdr_chain_set_gain_channels(self.h, C.c_uint32(first_channel), C.c_uint32(g.size), _hp(g) if g.size else None))

    def set_agc(self, agc_on=None, agc_on_all=0):
        """which receivers AGC() steps behind every process(): agc_on int32 [channels] of 0 (held) / 1 (stepped), or None: agc_on_all for all
        (msdr_chain_set_agc)"""
        a = np.ascontiguousarray(agc_on, np.int32) if agc_on is not None else None
        if a is not None and a.size != self.channels:
            raise ValueError("set_agc: %d values for %d channels" % (a.size, self.channels))
        _ck(self.ctx.lib.msdr_chain_set_agc(self.h, _hp(a), C.c_int32(agc_on_all)))

    def agc_state(self, channel):
        """a receiver's gain record behind every call so far (synchronises; msdr_chain_get_agc): multiplier (F32: the bits of the clamped
        gain), agc_idx, AGC_val, absmax of the last call, steps taken, agc_buffer[25], and the raw words"""
        w = np.zeros(AGC_STATE_WORDS, np.int32)
        _ck(self.ctx.lib.msdr_chain_get_agc(self.h, C.c_uint32(channel), _hp(w)))
        return {"multiplier": int(w[0]), "agc_idx": int(w[1]), "AGC_val": float(w[2:3].view(np.float32)[0]), "absmax": int(w[3]),
                "steps": int(w[4]), "agc_buffer": w[7:32].copy(), "words": w}

    def set_bank_post(self, on=True):
        """Synchronous AM and the LMS filter for the bank: once the chain is in phase-accumulator mode (set_nco_channels), its PLL demodulator
        and LMS filter run behind the per-receiver kernel on the pairs its I/Q twin stores, at fs / D, never through the auxiliary chain --
        which lets an fp32 chain with CHAIN_SYNCAM_PLL / LMS channels enter that mode and a Q15 one decimate.  Over a clear FIR history only,
        NCO mixer only, and for the rest of the chain's life (msdr_chain_set_bank_post)."""
        _ck(self.ctx.lib.msdr_chain_set_bank_post(self.h, C.c_int(1 if on else 0)))

    def bank_post(self):
        """whether the switch is on (msdr_chain_get_bank_post)"""
        on = C.c_int(0)
        _ck(self.ctx.lib.msdr_chain_get_bank_post(self.h, C.byref(on)))
        return bool(on.value)

    def set_pll_rate(self, sample_rate):
        """the rate the bank's PLL constants are evaluated for, from the next process() on: 0 = the reference's constants (the default), else
        fs / D as the caller sees fit; state kept; with set_bank_post on only (msdr_chain_set_pll_rate)"""
        _ck(self.ctx.lib.msdr_chain_set_pll_rate(self.h, C.c_double(float(sample_rate))))

    def pll_rate(self):
        """the rate in force, 0 = the reference's constants (msdr_chain_get_pll_rate)"""
        r = C.c_double(0.0)
        _ck(self.ctx.lib.msdr_chain_get_pll_rate(self.h, C.byref(r)))
        return r.value

    def pll_state(self, channel):
        """fil_out, omega2, phzerror of the channel's PLL behind every call so far (synchronises; msdr_chain_get_pll_state)"""
        st = np.zeros(3, np.float32)
        _ck(self.ctx.lib.msdr_chain_get_pll_state(self.h, C.c_uint32(channel), _hp(st)))
        return st

    def post_kernel(self):
        """msdr_chain_post_kernel: the PLL kernel of the last audio process() ("" where none ran)"""
        return _kernel_name(self.ctx.lib.msdr_chain_post_kernel, self.h)

    def set_block_kernel(self, on):
        """F32: a block-cadence call of a chain in per-channel mode as ONE launch (chain_f32pcb_kernel: demodulator, CMSIS-order cascade, int16
        conversion and the next history), bit-identical to the unfused launches, and capturable by graph().  Off by default; every state kept."""
        _ck(self.ctx.lib.msdr_chain_set_block_kernel(self.h, C.c_int(1 if on else 0)))

    def set_block_kernel_q15(self, on):
        """Q15: a block-cadence call of a chain in per-channel mode as ONE launch (chain_q15pcb_kernel: demodulator, the AudioFilterBiquad nodes from
        every channel's own records and the next history), bit-identical to the three unfused launches; a graph() tick is then one launch.  Off by
        default; every state kept."""
        _ck(self.ctx.lib.msdr_chain_set_block_kernel_q15(self.h, C.c_int(1 if on else 0)))

    def set_input_rows(self, rows, n_inputs=None):
        """One antenna stream (or a few) feeds the bank: channel c hears row rows[c] of a d_if that is [n_inputs, n] from the next process() /
        graph() on (integer array [channels]; n_inputs = rows.max() + 1 unless given).  rows = None: back to the identity, d_if [channels, n].
        Every state kept -- the FIR history stays the channel's own; the per-channel kernel family from the first call on."""
        if rows is None:
            _ck(self.ctx.lib.msdr_chain_set_input_rows(self.h, C.c_uint32(0), None))
            return
        r, ni = _input_rows("set_input_rows", rows, self.channels, n_inputs)
        _ck(self.ctx.lib.msdr_chain_set_input_rows(self.h, C.c_uint32(ni), _hp(r)))

    def fir_history(self, channel):
        """the raw int16 samples the chain carries for `channel`, oldest first; [hist_len, 2] pairs {I, Q} under set_complex_input
        (msdr_chain_get_fir_history)"""
        n = C.c_uint32(0)
        _ck(self.ctx.lib.msdr_chain_get_fir_history(self.h, C.c_uint32(channel), None, C.c_uint32(0), C.byref(n)))
        cx = hasattr(self.ctx.lib, "msdr_chain_get_complex_input") and self.complex_input()[0]
        h = np.zeros((n.value, 2) if cx else n.value, np.int16)
        _ck(self.ctx.lib.msdr_chain_get_fir_history(self.h, C.c_uint32(channel), _hp(h), C.c_uint32(h.size), None))
        return h

    def cmsis_state(self, channel):
        """pState of the cascade behind the kernel for `channel`: 4 floats per stage (msdr_chain_get_cmsis_state)"""
        st = np.zeros(4 * max(self.stages, 1), np.float32)
        _ck(self.ctx.lib.msdr_chain_get_cmsis_state(self.h, C.c_uint32(channel), _hp(st)))
        return st[:4 * self.stages]

    def set_node_coefficients(self, node, stage, coef):
        c = np.ascontiguousarray(coef, np.int32)
        if c.size != 5:
            raise ValueError("set_node_coefficients: one stage = 5 words (b0, b1, b2, a1, a2), %d given" % c.size)
        _ck(self.ctx.lib.msdr_chain_set_node_coefficients(self.h, C.c_uint32(node), C.c_uint32(stage), _hp(c)))

    def set_node_coefficients_channels(self, node, first_channel, stage, coefs):
        """setCoefficients(stage, coefs[i]) on biquad node `node` of channel first_channel + i only: coefs int32 [count, 5]."""
        c = _coefs_per_channel("set_node_coefficients_channels", coefs)
        _ck(self.ctx.lib.msdr_chain_set_node_coefficients_channels(self.h, C.c_uint32(node), C.c_uint32(first_channel), C.c_uint32(c.shape[0]),
                                                                   C.c_uint32(stage), _hp(c)))

    def set_biquad_coeffs(self, coeffs):
        c = np.ascontiguousarray(coeffs, np.float32).reshape(-1)
        if self.stages and c.size != 5 * self.stages:
            raise ValueError("set_biquad_coeffs: %d values given, the chain's cascade has %d stages x 5" % (c.size, self.stages))
        _ck(self.ctx.lib.msdr_chain_set_biquad_coeffs(self.h, _hp(c)))

    def set_biquad_coeffs_channels(self, first_channel, coeffs):
        """F32: channel first_channel + i gets cascade coefficients of its own, coeffs[i] (float32 [count, stages, 5] or [count, 5 * stages]);
        every state kept; the cascade runs in CMSIS order behind the demodulator kernel (biquad_df1_seq_pc_kernel) from the first call on."""
        c = _cascade_per_channel("set_biquad_coeffs_channels", coeffs, self.stages)
        _ck(self.ctx.lib.msdr_chain_set_biquad_coeffs_channels(self.h, C.c_uint32(first_channel), C.c_uint32(c.shape[0]), _hp(c)))

    def node_kernel(self):
        """msdr_chain_node_kernel: the kernel that ran the biquad nodes in the last process() ("" for no nodes, fp32 chains, before the first call)."""
        return _kernel_name(self.ctx.lib.msdr_chain_node_kernel, self.h)

    def info(self):
        i = ChainInfo()
        _ck(self.ctx.lib.msdr_chain_get_info(self.h, C.byref(i)))
        return {"kernel": i.kernel.decode(), "grid": i.grid, "block": i.block, "lds_bytes": i.lds_bytes,
                "time_segments": i.time_segments, "warmup": i.warmup, "tile": i.tile, "taps_padded": i.taps_padded,
                "mfma_ksteps": i.mfma_ksteps, "env_scan": i.env_scan, "flavour": i.flavour}

    def geometry(self):
        """msdr_chain_get_geometry: the constant run geometry the last process() ran with on the wave-stream kernels, 0 = read from the table headers"""
        g = C.c_uint32(0)
        _ck(self.ctx.lib.msdr_chain_get_geometry(self.h, C.byref(g)))
        return g.value

    def iq_shared(self):
        """msdr_chain_get_iq_shared: 1 where the last process() ran its envelope launch with Q on accumulator 0's tap fragments"""
        g = C.c_uint32(0)
        _ck(self.ctx.lib.msdr_chain_get_iq_shared(self.h, C.byref(g)))
        return g.value

    def enable_timing(self, on=True):
        _ck(self.ctx.lib.msdr_chain_enable_timing(self.h, int(on)))

    def kernel_time(self, reset=True):
        ms, n = C.c_double(0), C.c_uint64(0)
        _ck(self.ctx.lib.msdr_chain_get_kernel_time(self.h, C.byref(ms), C.byref(n), int(reset)))
        return ms.value, n.value


GATHER_SLOTS = 4


def comm_unique_id():
    """128 opaque bytes made by rank 0 (ncclGetUniqueId); pass them to the other ranks by any host channel."""
    buf = C.create_string_buffer(128)
    _ck(load_library().msdr_comm_get_unique_id(buf))
    return buf.raw


class Comm:
    """msdr_comm_*: the RCCL gather of demodulated audio, driven from C (include/msdr.h)."""

    def __init__(self, ctx, unique_id, rank, world):
        self.ctx, self.rank, self.world = ctx, rank, world
        h = _p()
        _ck(ctx.lib.msdr_comm_create(ctx.h, C.c_char_p(unique_id), int(rank), int(world), C.byref(h)))
        self.h = h

    def begin(self, slot, d_local_ptr, local_bytes, d_recv_ptr, root):
        _ck(self.ctx.lib.msdr_gather_audio_begin(self.h, int(slot), _p(d_local_ptr), C.c_size_t(local_bytes),
                                                 _p(d_recv_ptr) if d_recv_ptr else None, int(root)))

    def wait(self, slot, host_wait=False):
        _ck(self.ctx.lib.msdr_gather_audio_wait(self.h, int(slot), int(host_wait)))

    def close(self):
        if getattr(self, "h", None):
            if getattr(self.ctx, "h", None):
                self.ctx.lib.msdr_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
