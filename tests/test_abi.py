"""CPU-side checks of the product library: it builds/loads, exports every symbol include/msdr.h
declares, its host-side designers match the reference-generated golden vectors bit for bit, and
it FAILS LOUDLY (no CPU fallback) when no GPU is present."""
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
import orclib  # noqa: E402
import reflive  # noqa: E402


def declared_functions():
    names = set()
    for header in ("msdr.h", "msdr_cmsis.h"):
        src = open(os.path.join(ROOT, "include", header)).read()
        src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
        src = "\n".join(l for l in src.splitlines() if not l.lstrip().startswith("#"))      # macro lines are not declarations
        names |= set(re.findall(r"\b(msdr_[a-zA-Z0-9_]+)\s*\(", src))
    return sorted(names)


def test_library_exports_every_declared_symbol():
    lib = msdr.load_library()
    names = declared_functions()
    assert len(names) >= 40
    missing = [n for n in names if not hasattr(lib, n)]
    assert missing == []


def test_no_oracle_or_reference_linked_into_product():
    out = subprocess.check_output(["nm", "-D", msdr.LIB_PATH]).decode()
    assert "orc_" not in out and not re.search(r"\b[TtWw] arm_", out)          # (msdr_arm_* are the library's own CMSIS-signature shims)
    ldd = subprocess.check_output(["ldd", msdr.LIB_PATH]).decode()
    assert "liboracle" not in ldd and "msdr_ref" not in ldd
    for root, _, files in os.walk(os.path.join(ROOT, "minimal-sdr_amd")):
        for f in files:
            if f.endswith((".hip", ".hiph", ".cpp", ".h", ".py")):
                text = open(os.path.join(root, f)).read()
                assert "liboracle" not in text and "msdr_oracle" not in text and "orclib" not in text, f


def test_chain_info_struct_matches_the_header():
    """msdr_chain_info grew by `flavour`: the ctypes mirror has the header's fields in the header's order, and every MSDR_FLAVOUR_* value."""
    hdr = open(os.path.join(ROOT, "include", "msdr.h")).read()
    st = hdr[hdr.rindex("typedef struct", 0, hdr.index("} msdr_chain_info;")):hdr.index("} msdr_chain_info;")]
    st = re.sub(r"/\*.*?\*/", "", st, flags=re.S)
    fields = []
    for decl in re.findall(r"(?:char|uint32_t)\s+([^;]+);", st):
        fields += [re.sub(r"\[.*\]", "", f).strip() for f in decl.split(",")]
    assert fields == [f[0] for f in msdr.ChainInfo._fields_], fields
    assert fields[-2:] == ["env_scan", "flavour"]
    assert C.sizeof(msdr.ChainInfo) == 64 + 4 * (len(fields) - 1)
    for name, val in re.findall(r"#define MSDR_(FLAVOUR_[A-Z_]+)\s+(0x[0-9a-fA-F]+|\d+)u?\b", hdr):
        assert getattr(msdr, name) == int(val, 0), name
    assert len(re.findall(r"#define MSDR_FLAVOUR_[A-Z_]+\s", hdr)) == 13


class ArmFirQ15(C.Structure):          # include/msdr_cmsis.h = arm_math.h:1027-1032
    _fields_ = [("numTaps", C.c_uint16), ("pState", C.c_void_p), ("pCoeffs", C.c_void_p)]


def test_cmsis_shim_init_contract_without_a_device():
    """msdr_arm_fir_init_q15 keeps arm_fir_init_q15's contract (arm_fir_init_q15.c:93-109): odd numTaps -> ARGUMENT_ERROR and the
    instance untouched; otherwise the three fields are bound and numTaps + blockSize state samples cleared.  Without a bound
    context there is nothing to run on, and the status says so (no CPU path)."""
    lib = msdr.load_library()
    lib.msdr_arm_fir_init_q15.argtypes = [C.c_void_p, C.c_uint16, C.c_void_p, C.c_void_p, C.c_uint32]
    assert lib.msdr_cmsis_bind(None, 0) == 0
    S = ArmFirQ15(7, 1234, 5678)
    coef = np.arange(1, 103, dtype=np.int16)
    state = np.full(102 + 128 + 4, 77, np.int16)
    assert lib.msdr_arm_fir_init_q15(C.byref(S), 101, coef.ctypes.data, state.ctypes.data, 128) == -1
    assert (S.numTaps, S.pState, S.pCoeffs) == (7, 1234, 5678) and (state == 77).all()
    assert lib.msdr_arm_fir_init_q15(C.byref(S), 102, coef.ctypes.data, state.ctypes.data, 128) == -1      # no context bound
    assert (S.numTaps, S.pState, S.pCoeffs) == (102, state.ctypes.data, coef.ctypes.data)
    assert (state[:230] == 0).all() and (state[230:] == 77).all()
    lib.msdr_arm_fir_fast_q15(C.byref(S), None, None, 128)          # unknown instance: returns, nothing to do


def test_designer_fir_matches_golden(golden):
    for (n, fc, a, t, dfc) in golden.meta["design_cases"]:
        want = golden["design/n%d_fc%d_a%d_t%d_d%d_pif" % (n, fc, a, t, dfc)]
        got = msdr.calc_fir_coeffs(n, fc, a, t, dfc, 24000.0, room=want.size)
        assert np.array_equal(got, want), (n, fc, a, t, dfc)


def test_designer_fir_matches_oracle_random(orc):
    rng = np.random.default_rng(21)
    differ = 0
    # three designs where the two PIs give different taps (about 1.4 % of random designs do: 1 LSB in a tap pair), then random ones
    cases = [(504, 7945.0, 70.0, 0, 1592.0), (206, 8477.0, 30.0, 0, 1690.0), (250, 7163.0, 10.0, 1, 483.0)]
    for _ in range(80):
        n = int(rng.integers(4, 520)) & ~1
        fc, a = float(rng.integers(100, 9000)), float(rng.choice([10.0, 30.0, 45.5, 50.0, 70.0, 90.0]))
        cases.append((n, fc, a, int(rng.integers(0, 5)), float(rng.integers(50, 2000))))
    for n, fc, a, t, dfc in cases:
        pif = msdr.calc_fir_coeffs(n, fc, a, t, dfc)
        pid = msdr.calc_fir_coeffs(n, fc, a, t, dfc, pi_double=True)
        assert np.array_equal(pif, orc.calc_fir_coeffs(n, fc, a, t, dfc))
        assert np.array_equal(pid, orc.calc_fir_coeffs(n, fc, a, t, dfc, pi_double=True))
        assert np.abs(pif.astype(np.int32) - pid).max() <= 2
        differ += int(not np.array_equal(pif, pid))
    assert differ >= 3             # the two PIs are distinguishable: this test would notice a swapped flag


def test_designer_fir_both_pi_variants_match_the_compiled_reference():
    """msdr_calc_FIR_coeffs = the sketch with the vendored header's float PI; msdr_calc_FIR_coeffs_pid = with Arduino.h's
    double literal (what the Teensy binary computes).  Both against the reference's own source built with that PI: its recorded
    answers (tests/reflive.py), and the compiled reference itself where it is built."""
    for d in reflive.answers("designer_wide"):
        assert len(d["params"]) == 60
        for i, (n, fc, a, t, dfc) in enumerate(d["params"]):
            n, t = int(n), int(t)
            for pid in (False, True):
                want = d["c%d_%s" % (i, reflive.PI[pid])]
                got = msdr.calc_fir_coeffs(n, fc, a, t, dfc, 24000.0, room=want.size, pi_double=pid)
                assert np.array_equal(got, want), (n, fc, a, t, dfc, pid)


def test_designer_biquad_matches_oracle_and_survey(orc):
    corr = msdr.AUDIO_SAMPLE_RATE_EXACT / 24000.0
    lp = msdr.biquad_design(msdr.BQ_LOWPASS, np.float32(5400 * corr), 0.54)
    assert list(lp) == [236552419, 473104839, 236552419, -175469220, 47937074]   # SURVEY appendix, before negation
    rng = np.random.default_rng(3)
    for kind in range(6):
        for _ in range(20):
            f = float(rng.uniform(50, 20000))
            q = float(rng.uniform(0.3, 20)) if kind < 4 else float(rng.uniform(-12, 12))
            sl = float(rng.uniform(0.3, 1.0))
            assert np.array_equal(msdr.biquad_design(kind, f, q, sl), orc.biquad_design(kind, f, q, sl)), (kind, f, q, sl)


def test_no_cpu_fallback_without_gpu():
    """On a box without a HIP device the library must refuse to create a context (and says why)."""
    lib = msdr.load_library()
    if lib.msdr_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(msdr.MsdrError) as e:
        msdr.Context(0)
    assert e.value.status == msdr.STATUS_NO_DEVICE
    assert "no CPU path" in str(e.value)
    assert lib.msdr_fir_q15_process(None, None, None, 128) != 0
    assert lib.msdr_chain_process(None, None, None, 128) != 0


def test_rfft128_tables_match_reference_tables(golden):
    """Row f4: the product regenerates the three CMSIS tables from their formulas; here they meet the reference's literals."""
    tw, a, b = msdr.rfft128_tables()
    assert np.array_equal(tw, golden["fft/twiddleCoef_64_q15"])
    assert np.array_equal(a, golden["fft/realCoefAQ15_stride64"])
    assert np.array_equal(b, golden["fft/realCoefBQ15_stride64"])


def test_rfft_init_check_mirrors_arm_rfft_init_q15():
    lib = msdr.load_library()
    assert lib.msdr_rfft_q15_init_check(128, 0, 1) == 0
    for n in (0, 16, 100, 129, 16384):                       # arm_rfft_init_q15.c:2217-2220
        assert lib.msdr_rfft_q15_init_check(n, 0, 1) == msdr.STATUS_ARGUMENT_ERROR
    for n in (32, 64, 256, 8192):                            # valid for CMSIS, not built here
        assert lib.msdr_rfft_q15_init_check(n, 0, 1) == -2
    assert lib.msdr_rfft_q15_init_check(128, 1, 1) == -2


def test_cascade_info_routes_the_reference_cascade_to_the_parallel_solver(orc):
    """msdr_biquad_df1_f32_cascade_info (host only): the reference's LP + notch cascade and the Linkwitz-Riley set stay on the
    block-parallel IIR, high-pass pairs and narrow low-frequency notches go to CMSIS order."""
    corr = orclib.AUDIO_SAMPLE_RATE_EXACT / 24000.0
    LP, HP, NT = orclib.BQ_LOWPASS, orclib.BQ_HIGHPASS, orclib.BQ_NOTCH

    def rows(specs):
        out = []
        for kind, f, q in specs:
            c = orc.biquad_design(kind, np.float32(f), q).astype(np.float64) / 2 ** 30
            out.append([c[0], c[1], c[2], -c[3], -c[4]])
        return np.array(out, np.float32)

    k, nz, seq = msdr.biquad_cascade_info(rows([(LP, 5400 * corr, 0.54), (NT, 3000 * corr, 15.0)]))      # Minimal-SDR.ino:356, :391-393
    assert 15 < k < 25 and 1e-7 < nz < 1e-6 and not seq
    k, nz, seq = msdr.biquad_cascade_info(rows([(LP, 5400 * corr, q) for q in (0.54, 1.3, 0.54, 1.3)]))   # .ino:393-399
    assert k < 10 and not seq
    assert msdr.biquad_cascade_info(rows([(HP, 300.0, 0.707)]))[2]
    assert msdr.biquad_cascade_info(rows([(HP, 300.0, 0.707)] * 2))[0] > 1e4
    assert msdr.biquad_cascade_info(rows([(NT, 300.0, 20.0), (LP, 5000.0, 0.7)]))[2]
    assert msdr.biquad_cascade_info(np.zeros((0, 5), np.float32)) == (1.0, 0.0, False)


def test_python_setters_refuse_arrays_of_the_wrong_length():
    """the C setters copy num_taps / osc_len / 5 x stages elements from the caller's pointer; the ctypes wrappers must not hand
    them a shorter numpy array (a host out-of-bounds read that becomes the live filter).  Checked on the class methods without a device."""
    import inspect
    sys.path.insert(0, os.path.join(ROOT, "minimal-sdr_amd", "python"))
    import msdr
    for cls, names in ((msdr.Chain, ("set_taps", "set_osc", "set_biquad_coeffs", "set_node_coefficients")),
                       (msdr.FirQ15, ("set_coeffs",)), (msdr.FirF32, ("set_coeffs",)), (msdr.BiquadDf1F32, ("set_coeffs",))):
        for n in names:
            assert "raise ValueError" in inspect.getsource(getattr(cls, n)), (cls.__name__, n)
    # and one of them end to end on an object that never reaches the library
    c = msdr.Chain.__new__(msdr.Chain)
    c.arith, c.ntaps, c.osc_len, c.stages = msdr.ARITH_F32, 102, 128, 2
    import numpy as np
    import pytest
    with pytest.raises(ValueError):
        c.set_taps(0, np.zeros(50, np.float32), np.zeros(102, np.float32))
    with pytest.raises(ValueError):
        c.set_osc(np.zeros(64, np.float32), np.zeros(64, np.float32))
    with pytest.raises(ValueError):
        c.set_biquad_coeffs(np.zeros(5, np.float32))
