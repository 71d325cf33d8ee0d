"""The cases of the per-channel fp32 cascade tests, shared by tests/test_gpu_cascade_per_channel_f32.py (GPU) and tests/test_cascade_pc_cases.py
(the CPU-side conditions on them): the designer family, the inputs, a stateful arm_biquad_cascade_df1_f32 of the oracle whose pCoeffs can be
rewritten over its kept pState, and float64 references of streams whose cascade coefficients change.

The cascades are the reference's own designer's (AudioFilterBiquad's setLowpass / setNotch through the oracle, as f32pc_cases.sections()):
low-pass Q 0.54 + notch Q 15 at 3000 and 4000 Hz, + notch Q 2 at 1500 Hz, and the low-pass alone.  The notches Q 15 at 400 and 1000 Hz belong
to the stage tests' pool only (they compare with the oracle's own fp32 arithmetic): behind the chain the ORACLE leaves the level-1 clause
e_orc <= fp32_noise + 1e-6 with them on the bank's own input (400 Hz: 1.196e-5 against 1.142e-5 on channel 60; 1000 Hz: 3.239e-6 against
3.190e-6 on channel 15), so the chain tests' family goes without them."""
import ctypes as C

import numpy as np

import orclib
from f32judge import truth64
from f32pc_cases import B, CORR, FS4, NT, bw_taps, hilbert_pair  # noqa: F401

AM, LSB, USB = orclib.AM, orclib.LSB, orclib.USB
NOTCHES = ((400.0, 15.0), (1000.0, 15.0), (3000.0, 15.0), (4000.0, 15.0), (1500.0, 2.0))          # the stage tests' pool
CHAIN_NOTCHES = NOTCHES[2:]                                                                        # the chain tests' family
PASS = np.array([1, 0, 0, 0, 0], np.float32)          # a section that passes its input: "the low-pass alone" in a two-stage cascade
_ORC = []


def _orc():
    if not _ORC:
        _ORC.append(orclib.Oracle())
    return _ORC[0]


def section(kind, f, q):
    """one designer section as a {b0, b1, b2, -a1, -a2} row (the formula of f32pc_cases.sections())"""
    c = np.asarray(_orc().biquad_design(kind, np.float32(f * CORR), q), np.float64) / 1073741824.0
    return np.array([c[0], c[1], c[2], -c[3], -c[4]], np.float32)


def lowpass():
    return section(orclib.BQ_LOWPASS, 5400.0, 0.54)


def notch(f, q):
    return section(orclib.BQ_NOTCH, f, q)


def family():
    """the four two-stage cascades of the chain tests: low-pass + each notch, and the low-pass alone"""
    lp = lowpass()
    return [np.stack([lp, notch(f, q)]) for f, q in CHAIN_NOTCHES] + [np.stack([lp, PASS])]


def lp_notch3k():
    """the reference's own pair (f32pc_cases.cascade("lp+notch")): well conditioned, block-parallel as a uniform cascade"""
    return np.stack([lowpass(), notch(3000.0, 15.0)])


def bank_rows(ch, offset=0):
    """the family dealt round a bank of ch channels: [ch, 2, 5]"""
    fam = family()
    return np.stack([fam[(c + offset) % len(fam)] for c in range(ch)])


def stage_rows(ch, stages, offset=0):
    """[ch, stages, 5] for the stage tests: sections drawn from the family's pool (low-pass, the five notches), a different draw per channel"""
    pool = [lowpass()] + [notch(f, q) for f, q in NOTCHES]
    return np.stack([np.stack([pool[(c + offset + 2 * s) % len(pool)] for s in range(stages)]) for c in range(ch)])


def highpass_pair():
    """the cascade the differential tests rely on: two 300 Hz high-pass sections, which every instance runs in CMSIS order"""
    hp = section(orclib.BQ_HIGHPASS, 300.0, 0.7071)
    return np.stack([hp, hp])


def signal(seed, ch, n):
    return np.random.default_rng(seed).integers(-20000, 20001, (ch, n)).astype(np.int16)


def audio(seed, ch, n):
    """what a cascade stage is fed: white noise with a DC term, as an envelope has"""
    r = np.random.default_rng(seed)
    return (0.25 + 0.2 * r.standard_normal((ch, n))).astype(np.float32)


class Df1:
    """arm_biquad_cascade_df1_f32 of the oracle with its instance kept: run() carries pState, set_coeffs() rewrites pCoeffs in place."""

    def __init__(self, coeffs):
        self.c = np.array(coeffs, np.float32).reshape(-1)
        self.ns = self.c.size // 5
        self.st = np.zeros(4 * self.ns, np.float32)
        self.S = orclib.BiquadDf1()
        _orc().lib.orc_biquad_df1_init_f32(C.byref(self.S), C.c_uint8(self.ns), self.c.ctypes.data_as(C.c_void_p), self.st.ctypes.data_as(C.c_void_p))

    def set_coeffs(self, coeffs):
        self.c[:] = np.asarray(coeffs, np.float32).reshape(-1)

    def run(self, x):
        x = np.ascontiguousarray(x, np.float32)
        y = np.empty_like(x)
        _orc().lib.orc_biquad_df1_f32_run(C.byref(self.S), x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), C.c_uint32(x.size))
        return y


def df1_64(d, plan):
    """the cascade in float64, direct form 1, over d; plan = [(first sample, coefficients [S, 5])...]: pCoeffs rewritten over the kept pState"""
    d = np.asarray(d, np.float64)
    y = np.empty_like(d)
    S = len(plan[0][1])
    st = np.zeros((S, 4))
    bounds = [p[0] for p in plan] + [d.size]
    for k, (_, cf) in enumerate(plan):
        cf = np.asarray(cf, np.float64)
        for t in range(bounds[k], bounds[k + 1]):
            v = d[t]
            for s in range(S):
                c, q = cf[s], st[s]
                acc = c[0] * v + c[1] * q[0] + c[2] * q[1] + c[3] * q[2] + c[4] * q[3]
                q[1], q[0], q[3], q[2] = q[0], v, q[2], acc
                v = acc
            y[t] = v
    return y


def stream_refs(x_row, mode, hi, hq, plan, osc=FS4):
    """(oracle, float64) of one channel's stream whose cascade coefficients change at the plan's boundaries, FIR and mixer unchanged"""
    st, want = {}, []
    bounds = [p[0] for p in plan] + [x_row.size]
    for k, (_, cf) in enumerate(plan):
        want.append(_orc().chain_f32(x_row[bounds[k]:bounds[k + 1]], int(mode), hi, hq, osc[0], osc[1], cf, state=st))
    return np.concatenate(want), df1_64(truth64(x_row, int(mode), hi, hq, osc[0], osc[1], None), plan)


def case_of(mode, hi, hq, bq, osc=FS4):
    return dict(mode=int(mode), hi=hi, hq=hq, oi=osc[0], oq=osc[1], bq=bq)


# ---- the chain tests' own shapes and inputs (the CPU-side conditions are checked on exactly these) ----
BANK_CH, BANK_N = 64, 6 * B                  # test 7
BOTH_CH, BOTH_N = 35, 6 * B                  # test 8
MOVE_CALL = 3 * B                            # test 9: 2 calls before the first per-channel call, 2 after


def bank_input():
    return signal(71, BANK_CH, BANK_N)


def both_input():
    return signal(81, BOTH_CH, BOTH_N)


def both_taps():
    return np.stack([bw_taps(600.0 + 100.0 * c) for c in range(BOTH_CH)])


def move_input():
    return signal(91, 2, 4 * MOVE_CALL)


def move_setup():
    """test 9: channel 0 an SSB channel on the Hilbert pair (its cascade's numerator folds into the taps), channel 1 an envelope channel"""
    ssb, am = hilbert_pair(NT), bw_taps(2400.0)
    return dict(sets_i=[am, ssb[0]], sets_q=[am, ssb[1]], modes=np.array([USB, AM], np.int32), tapsets=np.array([1, 0], np.int32),
                uniform=lp_notch3k(), rows=np.stack([family()[1], family()[2]]))
