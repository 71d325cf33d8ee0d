"""The model of the per-receiver gain and AGC (msdr_chain_set_gain / set_gain_channels / set_agc), in numpy, and what its tests share.

Q15, per receiver, at the full rate:
  freqconv (the oracle's mixer) -> the two ACCUMULATORS: an int64 dot product of each mixed stream with pCoeffs in CMSIS order (no reversal:
  pCoeffs[j] meets sample n - (numTaps - 1) + j), wrapped to int32 -- arm_fir_fast_q15's accumulator before its >> 15 -> the gained pair
  ssat16((int64(acc) * multiplier) >> 31) -> orc.demod_q15.  The ungained pair ssat16(acc >> 15) is what the meter sums.
F32: the oracle's fp32 FIR sums (orc.fir_f32_blocks) times the clamped gain, one fp32 multiply each -> orc.demod_f32.
After every call: absmax = min(32767, max(|I|, |Q|)) of the call's gained outputs (F32: (int) min(peak / in_scale, 32767) in fp32), then
one step of AGC() (Minimal-SDR.ino:479-513) restated here with every float operation rounded to fp32 -- tests/test_agc_model.py pins both
halves to the oracle (orc.fir_q15_blocks / chain_q15 at unity gain, orc.agc_block for the rule)."""
import numpy as np

B = 128
F = np.float32
RING = 25
IN_SCALE = F(1.0 / 32768.0)


def ssat16(v):
    return np.clip(v, -32768, 32767)


def multiplier(gain):
    """AudioAmplifier::gain, mixer.h:75-79"""
    n = F(gain)
    n = F(32767.0) if n > F(32767.0) else F(-32767.0) if n < F(-32767.0) else n
    return int(F(n * F(65536.0)))


def clamped(gain):
    n = F(gain)
    return F(32767.0) if n > F(32767.0) else F(-32767.0) if n < F(-32767.0) else n


def bits(v):
    return int(np.array([v], F).view(np.int32)[0])


def acc_q15(mixed, coeffs, hist=None):
    """the wrapping 32-bit accumulator of every output: int64 dot products, then the low 32 bits as a signed number"""
    c = np.asarray(coeffs, np.int64)
    h = np.zeros(c.size - 1, np.int64) if hist is None else np.asarray(hist, np.int64)
    xh = np.concatenate([h, np.asarray(mixed, np.int64)])
    acc = np.lib.stride_tricks.sliding_window_view(xh, c.size) @ c
    return ((acc + (1 << 31)) % (1 << 32) - (1 << 31)).astype(np.int32)


def pair_q15(acc, mult):
    """the gained int16 value of an accumulator (numpy's >> on int64 is arithmetic)"""
    return ssat16((np.asarray(acc, np.int64) * int(mult)) >> 31).astype(np.int16)


def plain_q15(acc):
    return ssat16(np.asarray(acc, np.int32) >> 15).astype(np.int16)


class Rx:
    """one receiver's record, as msdr_chain_get_agc returns it"""

    def __init__(self, f32=False, in_scale=IN_SCALE):
        self.f32, self.in_scale = f32, F(in_scale)
        self.val = F(1.0)
        self.ring = np.zeros(RING, np.int32)
        self.idx, self.absmax, self.steps, self.on = RING, 0, 0, 0
        self.branches = []          # what each step did, for the tests that must reach every branch

    @property
    def mult(self):
        return bits(clamped(self.val)) if self.f32 else multiplier(self.val)

    def set_gain(self, g):
        self.val = F(g)

    def words(self):
        w = np.zeros(32, np.int32)
        w[0], w[1], w[2], w[3], w[4] = self.mult, self.idx, bits(self.val), self.absmax, self.steps
        w[7:32] = self.ring
        return w

    def absmax_of(self, gi, gq):
        if gi.size == 0:
            return 0
        if self.f32:
            with np.errstate(over="ignore"):
                peak = F(max(np.abs(gi).max(), np.abs(gq).max()))
                return int(min(F(peak / self.in_scale), F(32767.0)))
        return int(min(32767, max(np.abs(gi.astype(np.int32)).max(), np.abs(gq.astype(np.int32)).max())))

    def after_call(self, absmax):
        """the step kernel: record the call's absmax; one AGC() step where AGC is on"""
        self.absmax = int(absmax)
        if self.on:
            self.steps += 1
            self.step(absmax)

    def step(self, absmax):
        """Minimal-SDR.ino:479-513"""
        tag = []
        self.idx -= 1
        if self.idx >= 0:
            self.ring[self.idx] = absmax
        else:
            self.idx = RING          # the store to agc_buffer[-1] is dropped
            tag.append("dropped")
        d = int(self.ring.sum()) // RING
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            f = F(F(16000.0) / F(d))
            if d == 0:
                tag.append("d0")
            v = self.val
            if float(f) > 1.3:
                fagc = F(v + F(F(v * f) / F(1500.0)))
                if fagc < F(40.0):
                    self.val = fagc
                    tag.append("up")
                else:
                    tag.append("max")
            elif float(v) > 0.1:
                for lim, div in ((0.6, 50.0), (0.7, 200.0), (0.8, 2000.0), (0.9, 4000.0)):
                    if float(f) < lim:
                        self.val = F(v - F(F(v * f) / F(div)))
                        tag.append("down%g" % div)
                        break
                else:
                    tag.append("dead")
            else:
                tag.append("floor")
        self.branches.append(tag)


def out_index(lo, hi, D=1):
    """the full-rate samples behind the outputs of one call over inputs [lo, hi)"""
    return np.arange(lo + D - 1, hi, D)


def mixed_q15(orc, xi, xq, si, sq, direction):
    """the mixer's two streams; a real input is xq = None (freq_conv with zeros on port 1, dir 1)"""
    if xq is None:
        return orc.freqconv_q15(xi, np.zeros_like(xi), si, sq, 1, 1)
    return orc.freqconv_q15(xi, xq, si, sq, direction, 1)


class BankQ15:
    """receivers on streams known in advance: the accumulators once, then call by call under the receivers' gains"""

    def __init__(self, orc, xi, xq, si, sq, modes, ti, tq, direction=0, rows=None, sqrt_kind=None):
        self.orc, self.modes, self.sqrt_kind = orc, modes, sqrt_kind
        ch = len(modes)
        self.rx = [Rx() for _ in range(ch)]
        self.acc = []
        for c in range(ch):
            r = c if rows is None else rows[c]
            mi, mq = mixed_q15(orc, xi[r], None if xq is None else xq[r], si[c], sq[c], direction)
            self.acc.append((acc_q15(mi, ti[c]), acc_q15(mq, tq[c])))

    def call(self, lo, hi, D=1, gain_on=True, n_valid=None):
        """-> (audio [ch, n_out], gained pairs [ch, n_out, 2], ungained sums of squares [ch]); steps every receiver"""
        idx = out_index(lo, hi if n_valid is None else lo + n_valid, D)
        audio, pairs, meter = [], [], []
        for c, rx in enumerate(self.rx):
            ai, aq = self.acc[c][0][idx], self.acc[c][1][idx]
            pi, pq = plain_q15(ai), plain_q15(aq)
            gi, gq = (pair_q15(ai, rx.mult), pair_q15(aq, rx.mult)) if gain_on else (pi, pq)
            a = self.orc.demod_q15(int(self.modes[c]), gi, gq) if self.sqrt_kind is None else self.orc.demod_q15(int(self.modes[c]), gi, gq, self.sqrt_kind)
            audio.append(a)
            pairs.append(np.stack([gi, gq], axis=-1))
            meter.append(int((pi.astype(np.int64) ** 2 + pq.astype(np.int64) ** 2).sum()))
            if gain_on:
                rx.after_call(rx.absmax_of(gi, gq))
        return np.stack(audio), np.stack(pairs), np.array(meter, np.uint64)


def check_words(chain, rxs, tag=""):
    """msdr_chain_get_agc of every receiver against the model's records: words 0 .. 4, 5 .. 6 zero, the ring"""
    for c, rx in enumerate(rxs):
        got, want = chain.agc_state(c)["words"], rx.words()
        assert np.array_equal(got, want), (tag, c, got.tolist(), want.tolist())


def nco_rows(steps, phases, n):
    """(osc_i "sin", osc_q "cos") [ch, n] of phase-accumulator oscillators: the library's host-side msdr_nco_q15"""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "minimal-sdr_amd", "python"))
    import msdr
    ph = (np.asarray(phases, np.uint64)[:, None] + np.arange(n, dtype=np.uint64)[None, :] * np.asarray(steps, np.uint64)[:, None]) & np.uint64(0xFFFFFFFF)
    s, c = msdr.nco_q15(ph.astype(np.uint32))
    return s.reshape(ph.shape), c.reshape(ph.shape)


def corners(lowpass_taps):
    """The corners of the gain arithmetic as one bank of four AM / LSB / USB / AM receivers, 256 samples (what tests/test_agc_model.py asserts of it):
      0  all-32767 taps, a constant -32768 input, oscillator at phase 0 (cos 32767): the accumulator WRAPS; gain 0.25
      1  the same at phase 2^29 (cos = sin = 23170): wraps in both streams; a NEGATIVE gain, -2.5
      2  a loud random input behind the low-pass; gain 0: a ZERO multiplier
      3  the same input; gain 40: SATURATED outputs at both ends"""
    rng = np.random.default_rng(77)
    n, nt = 256, len(lowpass_taps)
    x = np.full((4, n), -32768, np.int16)
    x[2:] = rng.integers(-30000, 30001, n)
    taps = np.stack([np.full(nt, 32767, np.int16)] * 2 + [np.asarray(lowpass_taps, np.int16)] * 2)
    steps = np.array([0, 0, 0x0C000001, 0x0C000001], np.uint64)
    phases = np.array([0, 0x20000000, 5, 5], np.uint64)
    return dict(x=x, taps=taps, steps=steps, phases=phases, gains=(0.25, -2.5, 0.0, 40.0), modes=np.array([1, 2, 3, 1], np.int32), n=n)
