"""Per-receiver gain and AGC of the down-converter bank (F32): msdr_chain_set_gain / set_gain_channels / set_agc / get_agc on fp32 chains.

The plan of tests/test_gpu_agc_per_channel.py at its smallest shapes.  Model (tests/agc_model.py): the fp32 oracle's FIR sums of the mixed
streams (cx_cases.compose_f32; a real input is Q = 0, dir = 1) times the receiver's clamped gain, one fp32 multiply, then orc.demod_f32.
  audio    per receiver over the whole run, judged as the per-receiver fp32 chains are (tests/f32judge.py's two clauses at level 1, no cascade:
           e_go < 1e-5 against the fp32 model, e_gpu <= 2 e_orc + 1e-6 against the same chain in float64); the pairs to the same 1e-5; the
           meter to tests/test_gpu_meter_per_channel_f32.py's 2.5e-5 of the UNGAINED sum
  absmax   the device's within 1 of the model's: a relative error below 1e-5 of at most 32767 is below 1 before the truncation
  records  multiplier word (the bits of the clamped gain), agc_idx, AGC_val bits, steps and ring == the rule applied to the DEVICE'S OWN absmax
           sequence, after every call
Every figure is printed."""
import numpy as np
import pytest

import agc_model as M
import orclib
from cx_cases import compose_f32, compose_f64, interleave, pitch_of, rel
from gpuhelp import ctx, msdr  # noqa: F401
from test_gpu_decim_per_channel import step_list
from test_gpu_decim_per_channel_f32 import nco_chain
from test_gpu_nco_per_channel import Bank, off_grid_steps
from test_gpu_osc_per_channel_f32 import bw_taps, hilbert_pair, mixed_bank, signal

pytestmark = pytest.mark.gpu
B = 128
F, F64, U64, I16 = np.float32, np.float64, np.uint64, np.int16
GAIN = msdr.FLAVOUR_GAIN
GAINS = (0.0, -2.5, 0.25, 40.0, 37.5, 1.0, 3.0, 0.7, 12.0, -0.4, 1.5)


class BankF32:
    """the receivers' fp32 FIR sums once (and the same in float64), then call by call under the gains in the model's records"""

    def __init__(self, orc, xi, xq, si, sq, modes, ti, tq, direction=1, rows=None):
        self.orc, self.modes = orc, modes
        ch = len(modes)
        self.rx = [M.Rx(f32=True) for _ in range(ch)]
        self.f32, self.f64 = [], []
        for c in range(ch):
            r = c if rows is None else rows[c]
            a, b = xi[r], (np.zeros_like(xi[r]) if xq is None else xq[r])
            d = 1 if xq is None else direction
            self.f32.append(compose_f32(orc, a, b, si[c], sq[c], d, modes[c], ti[c], tq[c])[1:])
            self.f64.append(compose_f64(a, b, si[c], sq[c], d, modes[c], ti[c], tq[c])[1:])
        self.got, self.want32, self.want64 = ([[] for _ in range(ch)] for _ in range(3))

    def expect(self, c, idx):
        """(audio32, gained pair32, audio64, ungained sum of squares) of receiver c's outputs idx under its present gain"""
        g = M.clamped(self.rx[c].val)
        gi, gq = (self.f32[c][0][idx] * g).astype(F), (self.f32[c][1][idx] * g).astype(F)
        hi, hq = self.f64[c][0][idx] * float(g), self.f64[c][1][idx] * float(g)
        mode = int(self.modes[c])
        a64 = hi - hq if mode == 2 else hi + hq if mode == 3 else np.sqrt(hi * hi + hq * hq)
        e = float((self.f32[c][0][idx].astype(F64) ** 2 + self.f32[c][1][idx].astype(F64) ** 2).sum())
        return self.orc.demod_f32(mode, gi, gq), (gi, gq), a64, e


def gained(chain, bank, gains, agc_on):
    ch = len(bank.rx)
    chain.set_gain(True)
    chain.set_gain_channels(0, np.asarray(gains[:ch], F))
    chain.set_agc(np.asarray(agc_on[:ch], np.int32))
    for c, rx in enumerate(bank.rx):
        rx.set_gain(gains[c])
        rx.on = int(agc_on[c])
    M.check_words(chain, bank.rx, "before the first call")


def drive(ctx, chain, bank, x, step, D=1, iq=False, meter=False, tag="", audio=True):
    n, ch = x.shape[1], len(bank.rx)
    buf = met = None
    if iq:
        pitch = pitch_of(min(step, n) // D)
        buf = ctx.to_device(np.zeros((ch, pitch, 2), F))
        chain.set_iq_out(buf, pitch)
    if meter:
        met = ctx.to_device(np.zeros(ch, F64))
        chain.set_meter(met)
    for lo in range(0, n, step):
        m = min(step, n - lo)
        idx = M.out_index(lo, lo + m, D)
        dx = ctx.to_device(np.ascontiguousarray(x[:, lo:lo + m]))
        dy = ctx.array((ch, m // D), F) if audio else None
        chain.process(dx, dy, m)
        assert chain.info()["flavour"] & GAIN, chain.info()
        got = dy.download() if audio else None
        pairs = buf.download()[:, :m // D] if iq else None
        sums = met.download() if meter else None
        for c, rx in enumerate(bank.rx):
            a32, (gi, gq), a64, e = bank.expect(c, idx)
            if audio:
                bank.got[c].append(got[c]); bank.want32[c].append(a32); bank.want64[c].append(a64)
            if iq:
                den = float(np.sqrt((gi.astype(F64) ** 2 + gq.astype(F64) ** 2).sum()))
                err = float(np.sqrt(((pairs[c, :, 0].astype(F64) - gi) ** 2 + (pairs[c, :, 1].astype(F64) - gq) ** 2).sum()))
                print("agc f32 %s lo %d ch %d pairs %.3e" % (tag, lo, c, err / den if den else err))
                assert err <= 1e-5 * den, (tag, lo, c, err, den)
            if meter:
                print("agc f32 %s lo %d ch %d meter %.3e" % (tag, lo, c, abs(sums[c] - e) / e))
                assert abs(sums[c] - e) <= 2.5e-5 * e, (tag, lo, c, sums[c], e)
            dev = chain.agc_state(c)
            model_absmax = rx.absmax_of(gi, gq)
            print("agc f32 %s lo %d ch %d absmax device %d model %d" % (tag, lo, c, dev["absmax"], model_absmax))
            assert abs(dev["absmax"] - model_absmax) <= 1, (tag, lo, c, dev["absmax"], model_absmax)
            rx.after_call(dev["absmax"])          # the rule on the device's own absmax
        M.check_words(chain, bank.rx, "%s call at %d" % (tag, lo))


def judged(bank, tag):
    """the two clauses of tests/f32judge.py per receiver, over the receiver's whole run.  (cx_cases.judge_f32 also asks the ORACLE to be
    within 2e-6 of float64; the weak stations of the trajectory sit 50 dB under a carrier in the same fp32 sums, where the oracle itself is
    4.7e-6 of their level away)"""
    for c in range(len(bank.rx)):
        if bank.got[c]:
            got, want32, truth64 = np.concatenate(bank.got[c]), np.concatenate(bank.want32[c]), np.concatenate(bank.want64[c])
            e_go, e_gpu, e_orc = rel(got, want32), rel(got, truth64), rel(want32, truth64)
            print("agc f32 %s ch %d e_go %.3e e_gpu %.3e e_orc %.3e" % (tag, c, e_go, e_gpu, e_orc))
            assert e_go < 1e-5, (tag, c, e_go)
            assert e_gpu <= 2 * e_orc + 1e-6, (tag, c, e_gpu, e_orc)


def levels(rng, ch, n, weak=()):
    x = signal(rng, ch, n)
    for c in weak:
        x[c] = rng.integers(-300, 301, n)
    return x


# ------------------------------------------------------------------------------------------------ 1. every sliding-window geometry
def test_every_sliding_window_geometry(ctx, orc):
    rng = np.random.default_rng(9110)
    ch, n = 10, 6 * B
    modes, ti, tq = mixed_bank(ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=U64)
    si, sq = Bank(steps, phases).advance(n)
    x = levels(rng, ch, n, weak=(4, 8))
    for step, tile in ((B, 128), (2 * B, 256), (n, 512)):
        chain = nco_chain(ctx, ch, ti, tq, steps, phases, modes=modes)
        bank = BankF32(orc, x, None, si, sq, modes, ti, tq)
        gained(chain, bank, GAINS, [c & 1 for c in range(ch)])
        drive(ctx, chain, bank, x, step, tag="step %d" % step)
        info = chain.info()
        assert info["kernel"].startswith("chain_f32pcn_kernel") and info["tile"] == tile, info
        judged(bank, "step %d" % step)
        assert bank.rx[1].steps == n // step and bank.rx[0].steps == 0 and bank.rx[0].absmax == 0
        chain.close()


# ------------------------------------------------------------------------------------------------ 2. the tail and the segments
@pytest.mark.parametrize("n, segs", [(1001, 0), (4600, 0), (4600, 3)])
def test_the_tail_and_the_segments_and_the_peak_past_n(ctx, orc, n, segs):
    """the burst of tests/test_gpu_agc_per_channel.py in the last three samples: a peak that counted the outputs past n would be many times the model's"""
    rng = np.random.default_rng(9210 + n + segs)
    ch = 3
    modes = np.full(ch, orclib.AM, np.int32)
    ti = tq = np.stack([bw_taps(2800.0)] * ch)
    steps, phases = np.zeros(ch, U64), np.full(ch, 0x20000000, U64)
    si, sq = Bank(steps, phases).advance(n)
    x = rng.integers(-40, 41, (ch, n)).astype(I16)
    x[:, -3:] = 30000
    chain = nco_chain(ctx, ch, ti, tq, steps, phases, modes=modes, time_segments=segs)
    bank = BankF32(orc, x, None, si, sq, modes, ti, tq)
    gained(chain, bank, (1.0, 8.0, -3.0), (1, 1, 0))
    drive(ctx, chain, bank, x, n, iq=True, meter=True, tag="n %d segs %d" % (n, segs))
    info = chain.info()
    assert info["tile"] == 512 and info["time_segments"] == (1 if n == 1001 else segs or 2), info
    judged(bank, "n %d segs %d" % (n, segs))
    longer = BankF32(orc, np.concatenate([x, np.zeros((ch, 64), I16)], axis=1), None, *Bank(steps, phases).advance(n + 64), modes, ti, tq)
    past = longer.rx[0].absmax_of(*longer.expect(0, np.arange(n + 64))[1])
    assert past > 4 * bank.rx[0].absmax > 0, (past, bank.rx[0].absmax)
    chain.close()


# ------------------------------------------------------------------------------------------------ 3. decimation
@pytest.mark.parametrize("D", [2, 3, 8])
def test_decimation(ctx, orc, D):
    """read widths AL 2, 1, 4; 256 D inputs in calls of 32 and 128 outputs and one of 256 (4 / 4 / 2 channels per wave); I/Q buffer and meter set"""
    rng = np.random.default_rng(9310 + D)
    steps = step_list(rng)
    ch = steps.size
    modes, ti, tq = mixed_bank(ch)
    phases = rng.integers(0, 1 << 32, ch, dtype=U64)
    n = 256 * D
    x = levels(rng, ch, n, weak=(2, 5))
    si, sq = Bank(steps, phases).advance(n)
    for nout in (32, 128, 256):
        chain = nco_chain(ctx, ch, ti, tq, steps, phases, modes=modes)
        chain.set_decimation(D)
        bank = BankF32(orc, x, None, si, sq, modes, ti, tq)
        gained(chain, bank, GAINS, [1] * ch)
        drive(ctx, chain, bank, x, nout * D, D, iq=True, meter=True, tag="D %d nout %d" % (D, nout))
        info = chain.info()
        assert info["kernel"].startswith("chain_f32pcnd_kernel") and info["flavour"] & msdr.FLAVOUR_DECIMATED, info
        judged(bank, "D %d nout %d" % (D, nout))
        chain.close()


# ------------------------------------------------------------------------------------------------ 4. the AGC's trajectory
def test_agc_trajectory_on_one_shared_antenna_row(ctx, orc):
    """6 receivers on ONE input row with two carriers 50 dB apart, AGC on for four, 30 calls of 128.  A relative error needs audio with a
    level: the AM receivers sit on (or 200 Hz beside) their carrier, the USB / LSB receivers have the Hilbert pair of mixed_bank() and are
    tuned 700 Hz above / 1 kHz below theirs, the side whose sideband passes (a tone at the pair's level; with I and Q behind ONE low-pass,
    or tuned to the other side, I -+ Q cancels to 1 / 30 of the pair and any error is large against what is left).  The weak receivers sit
    50 dB under a carrier in the same fp32 sums: the oracle itself is 4.2e-6 .. 4.7e-6 of their level from float64 over the run (computed
    without a device; 8.4e-6 at most in any single call), inside the 1e-5 every receiver is held to."""
    rng = np.random.default_rng(9410)
    ch, calls = 6, 30
    n = calls * B
    t = np.arange(n)
    row = np.round(20000 * np.cos(2 * np.pi * 6000.0 * t / 24000.0) + 63 * np.cos(2 * np.pi * 2310.0 * t / 24000.0 + 1.0) + rng.normal(0, 1.5, n)).astype(I16)
    x = row[None, :]
    steps = np.array([msdr.nco_step(f) for f in (6000.0, 2310.0, 6700.0, 1310.0, 6000.0, 2110.0)], U64)
    phases = rng.integers(0, 1 << 32, ch, dtype=U64)
    modes = np.array([orclib.AM, orclib.AM, orclib.USB, orclib.LSB, orclib.AM, orclib.AM], np.int32)
    am = bw_taps(2800.0)
    ssb = hilbert_pair(am.size)          # passband 300 .. 1700 Hz
    ti, tq = np.stack([am, am, ssb[0], ssb[0], am, am]), np.stack([am, am, ssb[1], ssb[1], am, am])
    si, sq = Bank(steps, phases).advance(n)
    chain = nco_chain(ctx, ch, ti, tq, steps, phases, modes=modes)
    chain.set_input_rows(np.zeros(ch, np.uint32), 1)
    bank = BankF32(orc, x, None, si, sq, modes, ti, tq, rows=[0] * ch)
    gained(chain, bank, (4.0, 1.0, 20.0, 0.5, 2.0, 37.5), (1, 1, 1, 1, 0, 0))
    drive(ctx, chain, bank, x, B, tag="trajectory")
    judged(bank, "trajectory")
    seen = {t for rx in bank.rx for tag in rx.branches for t in tag}
    assert "dropped" in seen and "up" in seen and any(s.startswith("down") for s in seen), seen
    assert [rx.steps for rx in bank.rx] == [calls] * 4 + [0, 0] and bank.rx[1].val > 1.0 and bank.rx[4].val == F(2.0)
    assert chain.info()["flavour"] & msdr.FLAVOUR_SHARED_IF
    chain.close()


# ------------------------------------------------------------------------------------------------ 5. set_gain(1) alone; the flavour bit
@pytest.mark.parametrize("D", [1, 4])
def test_gain_on_with_nothing_else_set_changes_no_bit_and_the_flavour_bit(ctx, D):
    rng = np.random.default_rng(9510 + D)
    ch, n = 7, 256 * D
    modes, ti, tq = mixed_bank(ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=U64)
    x = signal(rng, ch, n)
    outs = []
    for on in (False, True, False):
        chain = nco_chain(ctx, ch, ti, tq, steps, phases, modes=modes)
        chain.set_decimation(D)
        chain.set_gain(on)
        if not on and len(outs) == 2:          # on, then off again: the state stays, the plain kernels run
            chain.set_gain(True)
            chain.set_gain_channels(0, np.full(ch, 5.0, F))
            chain.set_gain(False)
        pitch = pitch_of(n // D)
        buf, met = ctx.to_device(np.zeros((ch, pitch, 2), F)), ctx.to_device(np.zeros(ch, F64))
        chain.set_iq_out(buf, pitch)
        chain.set_meter(met)
        dy = ctx.array((ch, n // D), F)
        chain.process(ctx.to_device(x), dy, n)
        assert bool(chain.info()["flavour"] & GAIN) == on, chain.info()
        outs.append((dy.download(), buf.download(), met.download()))
        chain.close()
    for k in (1, 2):
        for a, b in zip(outs[0], outs[k]):
            assert np.array_equal(a.view(np.uint32 if a.dtype == F else U64), b.view(np.uint32 if b.dtype == F else U64)), k


# ------------------------------------------------------------------------------------------------ 6. meter, I/Q output, an I/Q-only call
def test_the_meter_is_ungained_the_pairs_are_gained_and_an_iq_only_call_steps(ctx, orc):
    rng = np.random.default_rng(9610)
    ch, n = 4, 3 * B
    modes, ti, tq = mixed_bank(ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=U64)
    si, sq = Bank(steps, phases).advance(n)
    x = signal(rng, ch, n)
    chain = nco_chain(ctx, ch, ti, tq, steps, phases, modes=modes)
    bank = BankF32(orc, x, None, si, sq, modes, ti, tq)
    gained(chain, bank, GAINS[:4], (1, 1, 1, 1))          # 0, -2.5, 0.25, 40: the meter is held to the ungained sum in drive()
    drive(ctx, chain, bank, x[:, :2 * B], B, iq=True, meter=True, tag="metered")
    before = [rx.steps for rx in bank.rx]
    chain.set_meter(None)
    bank2_x = x[:, 2 * B:]
    # an I/Q-only call through the same driver: no audio batch
    n0 = 2 * B
    pitch = pitch_of(B)
    buf = ctx.to_device(np.zeros((ch, pitch, 2), F))
    chain.set_iq_out(buf, pitch)
    chain.process(ctx.to_device(np.ascontiguousarray(bank2_x)), None, B)
    pairs = buf.download()[:, :B]
    for c, rx in enumerate(bank.rx):
        _, (gi, gq), _, _ = bank.expect(c, np.arange(n0, n0 + B))
        den = float(np.sqrt((gi.astype(F64) ** 2 + gq.astype(F64) ** 2).sum()))
        err = float(np.sqrt(((pairs[c, :, 0].astype(F64) - gi) ** 2 + (pairs[c, :, 1].astype(F64) - gq) ** 2).sum()))
        assert err <= 1e-5 * den, (c, err, den)
        dev = chain.agc_state(c)
        assert abs(dev["absmax"] - rx.absmax_of(gi, gq)) <= 1, c
        rx.after_call(dev["absmax"])
    M.check_words(chain, bank.rx, "behind the I/Q-only call")
    assert [rx.steps for rx in bank.rx] == [s + 1 for s in before]
    judged(bank, "metered")
    chain.close()


# ------------------------------------------------------------------------------------------------ 7. complex input, int16 audio
def test_complex_input_dir_0(ctx, orc):
    rng = np.random.default_rng(9710)
    ch, D = 5, 3
    n = 256 * D
    modes, ti, tq = mixed_bank(ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=U64)
    si, sq = Bank(steps, phases).advance(n)
    xi, xq = levels(rng, ch, n, weak=(1,)), levels(rng, ch, n, weak=(1,))
    chain = nco_chain(ctx, ch, ti, tq, steps, phases, modes=modes)
    chain.set_complex_input(True, 0)
    chain.set_decimation(D)
    bank = BankF32(orc, xi, xq, si, sq, modes, ti, tq, direction=0)
    gained(chain, bank, GAINS[1:], (1, 0, 1, 0, 1))
    drive(ctx, chain, bank, interleave(xi, xq), 128 * D, D, iq=True, meter=True, tag="complex")
    assert chain.info()["flavour"] & msdr.FLAVOUR_COMPLEX_IN
    judged(bank, "complex")
    chain.close()


def test_refusals(ctx):
    rng = np.random.default_rng(9910)
    ch = 3
    modes, ti, tq = mixed_bank(ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=U64)
    chain = nco_chain(ctx, ch, ti, tq, steps, phases, modes=modes)
    chain.set_gain_channels(0, np.array([1e9, -1e9, 2.0], F))          # clamped as AudioAmplifier::gain clamps
    w = [chain.agc_state(c) for c in range(ch)]
    assert [M.bits(F(v)) for v in (32767.0, -32767.0, 2.0)] == [s["multiplier"] for s in w] and w[0]["AGC_val"] == F(1e9)
    for f, a in ((chain.set_gain_channels, (2, [1.0, 1.0])), (chain.set_gain_channels, (0, [float("nan")])), (chain.set_agc, ([0, 1, 3],)), (chain.set_agc, (None, -1))):
        with pytest.raises(msdr.MsdrError) as e:
            f(*a)
        assert e.value.status == msdr.STATUS_ARGUMENT_ERROR
        assert [chain.agc_state(c)["words"].tolist() for c in range(ch)] == [s["words"].tolist() for s in w]
    chain.close()
