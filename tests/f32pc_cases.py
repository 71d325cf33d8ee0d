"""The cases of the per-channel fp32 chain tests, shared by tests/test_gpu_taps_per_channel_f32.py (GPU) and tests/test_f32pc_cases.py (the
CPU-side conditions on them): taps, mode, cascade, oscillator.  Taps are the designer's Q15 rows divided by 32768 at the bandwidth menu's
values (UI.cpp:332-345), as bank_taps of the Q15 test."""
import numpy as np

import orclib
from gpuhelp import msdr

B = 128
NT = 102
CORR = orclib.AUDIO_SAMPLE_RATE_EXACT / 24000.0
COS4, SIN4 = np.array([1, 0, -1, 0], np.float32), np.array([0, 1, 0, -1], np.float32)
FS4 = (SIN4, COS4)          # (osc_i, osc_q) of the Fs/4 mixer, for the oracle


def bw_taps(bw, n=NT):
    """calc_demod_filter(): calc_FIR_coeffs(FIR_AM_coeffs, numTaps, filter_bandwidth, 70, 0, 0.0, 24000), as floats"""
    return (msdr.calc_fir_coeffs(n, float(bw), 70.0, 0, 0.0, 24000.0)[:n].astype(np.float64) / 32768.0).astype(np.float32)


def bank_taps(ch, n=NT, lo=125.0, hi=5000.0):
    """ch distinct bandwidths of the menu's range (steps of 25 Hz from 125 to 5000 Hz)"""
    bws = np.round(np.linspace(lo, hi, ch) / 25.0) * 25.0 if ch <= 196 else lo + (np.arange(ch) % 196) * 25.0
    return np.stack([bw_taps(b, n) for b in bws])


def hilbert_pair(n, fc=1000.0, bw=1400.0):
    k = np.arange(n) - (n - 1) / 2
    proto = np.sinc(bw / 24000 * k) * np.kaiser(n, 6.0)
    proto /= proto.sum()
    return ((2 * proto * np.cos(2 * np.pi * fc / 24000 * k + np.pi / 4)).astype(np.float32),
            (2 * proto * np.cos(2 * np.pi * fc / 24000 * k - np.pi / 4)).astype(np.float32))


def nco128(cycles=3):
    """a table whose only period is its 128 entries"""
    k = np.arange(128)
    return ((np.round(32767 * np.sin(2 * np.pi * cycles * k / 128)).astype(np.int16) / 32768.0).astype(np.float32),
            (np.round(32767 * np.cos(2 * np.pi * cycles * k / 128)).astype(np.int16) / 32768.0).astype(np.float32))


def sections():
    """the reference's own low-pass (Q 0.54) and notch (Q 15), as {b0, b1, b2, -a1, -a2} rows"""
    orc = orclib.Oracle()

    def sec(kind, f, q):
        c = np.asarray(orc.biquad_design(kind, np.float32(f * CORR), q), np.float64) / 1073741824.0
        return np.array([c[0], c[1], c[2], -c[3], -c[4]], np.float32)
    return dict(lp=sec(orclib.BQ_LOWPASS, 5400.0, 0.54), notch=sec(orclib.BQ_NOTCH, 3000.0, 15.0))


def cascade(key):
    s = sections()
    return None if key is None else np.stack([s[k] for k in key.split("+")])


# every (taps, mode, cascade, oscillator) combination a judged GPU row uses: name -> (hi, hq, mode, cascade key, osc).  Where a GPU test runs a
# family of bandwidths (the bank, the rows 300 + 50 c Hz ...) the table holds the family's ends and its middle.
LONG_TAPS = (255, 511, 256, 512)          # tests/test_gpu_taps_per_channel_f32.py::test_long_tap_counts


def cases():
    out = {}
    A, L, U, C = orclib.AM, orclib.LSB, orclib.USB, orclib.CW
    ssb, cw = hilbert_pair(NT), hilbert_pair(NT, 700.0, 300.0)
    # the bank (tests 1, 1b, 5, 6, 8, 9, 10): AM, Fs/4, no cascade / low-pass / low-pass + notch
    for bw in (125.0, 2400.0, 5000.0):
        for key in (None, "lp", "lp+notch"):
            out["am_%d_%s" % (bw, key)] = (bw_taps(bw), bw_taps(bw), A, key, FS4)
    # the mixed bank (test 2): shared sets (AM 2400 / 1800, the SSB pair, the CW pair, each under LSB / USB / CW) beside own AM rows 300 .. 2000 Hz
    for bw in (300.0, 700.0, 1800.0, 2000.0):
        out["mixed_am_%d" % bw] = (bw_taps(bw), bw_taps(bw), A, None, FS4)
    for nm, pair in (("ssb", ssb), ("cw", cw)):
        for m in (L, U, C):
            out["mixed_%s_mode%d" % (nm, m)] = (pair[0], pair[1], m, None, FS4)
    # the general oscillator (test 3): both tables, AM rows 400 .. 3700 Hz, the SSB pair scaled by 1 - 0.01 c under LSB / USB / CW
    for cyc in (3, 5):
        for bw in (400.0, 1600.0, 2800.0):
            out["nco%d_am_%d" % (cyc, bw)] = (bw_taps(bw), bw_taps(bw), A, None, nco128(cyc))
        for m, sc in ((L, 0.99), (U, 0.98), (C, 0.97), (L, 0.95), (C, 0.89)):
            out["nco%d_mode%d_%.2f" % (cyc, m, sc)] = (ssb[0] * np.float32(sc), ssb[1] * np.float32(sc), m, None, nco128(cyc))
    # long filters (test 4): AM rows 500 .. 3500 Hz, the SSB pair under USB / LSB, Fs/4 and the oscillator table
    for n in LONG_TAPS:
        for osc_name, osc in (("fs4", FS4), ("nco", nco128())):
            for bw in (500.0, 1700.0, 3500.0):
                out["%dtaps_%s_am_%d" % (n, osc_name, bw)] = (bw_taps(bw, n), bw_taps(bw, n), A, None, osc)
            for m in (U, L):
                out["%dtaps_%s_mode%d" % (n, osc_name, m)] = (hilbert_pair(n)[0], hilbert_pair(n)[1], m, None, osc)
    # PLL / LMS channels (test 7): AM rows 1200 .. 3700 Hz, and what the PLL is fed: I + Q and I - Q of the same rows
    for bw in (1200.0, 1700.0, 3700.0):
        for m in (A, U, L):
            out["post_%d_mode%d" % (bw, m)] = (bw_taps(bw), bw_taps(bw), m, None, FS4)
    # the arm_fir_f32 stage (test 12) has its own gate (1e-6 against the oracle), not the chain's contract: no entry
    return out
