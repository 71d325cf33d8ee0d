"""Per-receiver gain and AGC of the down-converter bank (Q15): msdr_chain_set_gain / set_gain_channels / set_agc / get_agc.

Everything is compared with == against tests/agc_model.py (pinned to the oracle by tests/test_agc_model.py): the audio, the gained pairs in the
I/Q buffer, the ungained sums in the meter, and after EVERY call the record of every receiver (multiplier, agc_idx, AGC_val bits, absmax,
steps, the ring).  Oscillator model, banks and tiles are those of tests/test_gpu_nco_per_channel.py / test_gpu_decim_per_channel.py /
test_gpu_meter_per_channel.py."""
import numpy as np
import pytest

import agc_model as M
import orclib
from cx_cases import interleave, pitch_of
from gpuhelp import ctx, msdr  # noqa: F401
from test_gpu_decim_per_channel import NOUTS, TILES, nco_chain, step_list
from test_gpu_nco_per_channel import Bank, any_table, off_grid_steps, u32
from test_gpu_osc_per_channel import bw_taps, mixed_bank

pytestmark = pytest.mark.gpu
B = 128
I16, U64 = np.int16, np.uint64
AM, LSB, USB, CW, SYNCAM = orclib.AM, orclib.LSB, orclib.USB, orclib.CW, orclib.SYNCAM
ARG = msdr.STATUS_ARGUMENT_ERROR
GAINS = (0.0, -2.5, 0.25, 40.0, 37.5, 1.0, 3.0, 0.7, 12.0, -0.4, 1.5)          # the meter's four first; a zero multiplier, a negative gain


def refused(f, *a):
    with pytest.raises(msdr.MsdrError) as e:
        f(*a)
    assert e.value.status == ARG, e.value


def gained(chain, bank, gains, agc_on):
    """gain on, the receivers' gains and AGC switches set in chain and model"""
    ch = len(bank.rx)
    chain.set_gain(True)
    chain.set_gain_channels(0, np.asarray(gains[:ch], np.float32))
    chain.set_agc(np.asarray(agc_on[:ch], np.int32))
    for c, rx in enumerate(bank.rx):
        rx.set_gain(gains[c])
        rx.on = int(agc_on[c])
    M.check_words(chain, bank.rx, "before the first call")


def drive(ctx, chain, bank, x, step, D=1, iq=False, meter=False, tag="", audio=True, post=None, span=None):
    """calls of `step` INPUT samples over x (span = (lo, hi): over that stretch of it): after every call the audio, the pairs, the meter and
    every record equal the model's.  post(c, audio, pairs, lo): what runs behind the kernel on channel c's audio (PLL, LMS); -> the meters [calls, ch]"""
    first, n = span or (0, x.shape[1])
    ch = len(bank.rx)
    buf = met = None
    if iq:
        pitch = pitch_of(min(step, n - first) // D)
        buf = ctx.to_device(np.zeros((ch, pitch, 2), I16))
        chain.set_iq_out(buf, pitch)
    if meter:
        met = ctx.to_device(np.zeros(ch, U64))
        chain.set_meter(met)
    meters = []
    for lo in range(first, n, step):
        m = min(step, n - lo)
        dx = ctx.to_device(np.ascontiguousarray(x[:, lo:lo + m]))
        dy = ctx.array((ch, m // D), I16) if audio else None
        chain.process(dx, dy, m)
        want, pairs, sums = bank.call(lo, lo + m, D)
        if audio:
            got = dy.download()
            for c in range(ch):
                w = want[c] if post is None else post(c, want[c], pairs[c], lo)
                assert np.array_equal(got[c], w), (tag, lo, c)
        if iq:
            assert np.array_equal(buf.download()[:, :m // D], pairs), (tag, lo)
        if meter:
            assert np.array_equal(met.download(), sums), (tag, lo)
            meters.append(sums)
        M.check_words(chain, bank.rx, "%s call at %d" % (tag, lo))
    return np.stack(meters) if meters else None


def levels(rng, ch, n, weak=(0,)):
    """random IF rows; the receivers in `weak` get a few LSB behind the channel filter (+-300), the others nearly full scale"""
    x = rng.integers(-30000, 30001, (ch, n)).astype(I16)
    for c in weak:
        x[c] = rng.integers(-300, 301, n)
    return x


# ------------------------------------------------------------------------------------------------ 1. every sliding-window geometry
def test_every_sliding_window_geometry(ctx, orc, golden):
    """10 channels, 102 taps, AM / LSB / USB / CW; 6 calls of 128, 3 of 256, one of 768; every gain of GAINS, AGC on for every second receiver"""
    rng = np.random.default_rng(9100)
    ch, n = 10, 6 * B
    modes, ti, tq = mixed_bank(golden, ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=U64)
    si, sq = Bank(steps, phases).advance(n)
    x = levels(rng, ch, n, weak=(4, 8))
    agc_on = [c & 1 for c in range(ch)]
    for step, tile in ((B, 128), (2 * B, 256), (n, 512)):
        chain = nco_chain(ctx, ch, ti, tq, steps, phases, modes)
        bank = M.BankQ15(orc, x, None, si, sq, modes, ti, tq)
        gained(chain, bank, GAINS, agc_on)
        drive(ctx, chain, bank, x, step, tag="step %d" % step)
        info = chain.info()
        assert info["kernel"].startswith("chain_q15pcn_kernel") and info["tile"] == tile, info          # the names of the plain kernels
        assert bank.rx[1].steps == n // step and bank.rx[0].steps == 0
        assert any(abs(rx.absmax) == 32767 for rx in bank.rx) and bank.rx[0].absmax == 0          # saturated pairs; the zero multiplier
        chain.close()


def test_the_corners(ctx, orc):
    """agc_model.corners(): a wrapped accumulator under a gain and under a negative gain, a zero multiplier, outputs saturated at both ends
    (tests/test_agc_model.py asserts that the bank holds them); one call of 256 and two of 128, pairs and meter beside the audio"""
    k = M.corners(bw_taps(2800.0))
    si, sq = M.nco_rows(k["steps"], k["phases"], k["n"])
    for step in (256, 128):
        chain = nco_chain(ctx, 4, k["taps"], k["taps"], k["steps"], k["phases"], k["modes"])
        bank = M.BankQ15(orc, k["x"], None, si, sq, k["modes"], k["taps"], k["taps"])
        gained(chain, bank, k["gains"], (1, 1, 1, 1))
        drive(ctx, chain, bank, k["x"], step, iq=True, meter=True, tag="corners %d" % step)
        chain.close()


# ------------------------------------------------------------------------------------------------ 2. the tail and the segments
@pytest.mark.parametrize("n", [1001, 4600])
def test_the_tail_and_the_segments_and_the_peak_past_n(ctx, orc, golden, n):
    """3 channels, one call.  1001: tile 512, the second tile partly live.  4600: two time segments, one atomicMax each per receiver.  The IF is
    quiet but for a burst in its last three samples: the outputs inside the call meet it with the filter's edge taps, the outputs past n (same
    tile, never stored) with its centre -- a peak that counted them would be many times the model's."""
    rng = np.random.default_rng(9200 + n)
    ch = 3
    modes, ti, tq = mixed_bank(golden, ch)
    modes[:] = AM
    ti = tq = np.stack([bw_taps(2800.0)] * ch)
    steps, phases = np.zeros(ch, U64), np.full(ch, 0x20000000, U64)          # a constant oscillator: cos = sin = 23170
    si, sq = Bank(steps, phases).advance(n)
    x = rng.integers(-40, 41, (ch, n)).astype(I16)
    x[:, -3:] = 30000
    chain = nco_chain(ctx, ch, ti, tq, steps, phases, modes)
    bank = M.BankQ15(orc, x, None, si, sq, modes, ti, tq)
    gained(chain, bank, (1.0, 8.0, -3.0), (1, 1, 0))
    drive(ctx, chain, bank, x, n, iq=True, meter=True, tag="n %d" % n)
    info = chain.info()
    assert info["tile"] == 512 and (info["time_segments"] >= 2) == (n == 4600), info
    # what the peak would be with the outputs past n counted: the same stream followed by zeros
    longer = M.BankQ15(orc, np.concatenate([x, np.zeros((ch, 64), I16)], axis=1), None, *Bank(steps, phases).advance(n + 64), modes, ti, tq)
    longer.call(0, n + 64)
    assert longer.rx[0].absmax > 4 * bank.rx[0].absmax > 0, (longer.rx[0].absmax, bank.rx[0].absmax)
    chain.close()


# ------------------------------------------------------------------------------------------------ 3. decimation
@pytest.fixture(scope="module")
def dec_ref(golden):
    rng = np.random.default_rng(9300)
    steps = step_list(rng)
    ch = steps.size
    modes, ti, tq = mixed_bank(golden, ch)
    phases = rng.integers(0, 1 << 32, ch, dtype=U64)
    n = 768 * 8
    return dict(steps=steps, phases=phases, modes=modes, ti=ti, tq=tq, ch=ch, x=levels(rng, ch, n, weak=(2, 5)), osc=Bank(steps, phases).advance(n))


@pytest.mark.parametrize("D", [2, 3, 8])
def test_decimation(ctx, orc, dec_ref, D):
    """11 channels, 102 taps, mixed modes: 768 D inputs in calls of 32, 128, 256 outputs and one of 768, the tiles of
    tests/test_gpu_decim_per_channel.py (read widths AL 1, 0 and 4: one copy of the window, two copies, 16-byte reads); I/Q buffer and meter set"""
    r = dec_ref
    n = 768 * D
    x, (si, sq) = r["x"][:, :n], r["osc"]
    for nout, tile in zip(NOUTS, TILES[D]):
        chain = nco_chain(ctx, r["ch"], r["ti"], r["tq"], r["steps"], r["phases"], r["modes"])
        chain.set_decimation(D)
        bank = M.BankQ15(orc, x, None, si[:, :n], sq[:, :n], r["modes"], r["ti"], r["tq"])
        gained(chain, bank, GAINS, [1] * r["ch"])
        drive(ctx, chain, bank, x, nout * D, D, iq=True, meter=True, tag="D %d nout %d" % (D, nout))
        info = chain.info()
        assert info["kernel"].startswith("chain_q15pcnd_kernel") and info["tile"] == tile, info
        chain.close()


# ------------------------------------------------------------------------------------------------ 4. the AGC's trajectory
def test_agc_trajectory_on_one_shared_antenna_row(ctx, orc):
    """6 receivers hear ONE input row with two carriers 50 dB apart (20000 and 63 LSB); AGC on for four of them.  30 calls of 128: the ring turns
    over and the 26th store is dropped.  Records and audio after every call."""
    rng = np.random.default_rng(9400)
    ch, calls = 6, 30
    n = calls * B
    t = np.arange(n)
    f_strong, f_weak = 6000.0, 2310.0
    row = np.round(20000 * np.cos(2 * np.pi * f_strong * t / 24000.0) + 63 * np.cos(2 * np.pi * f_weak * t / 24000.0 + 1.0) + rng.normal(0, 1.5, n)).astype(I16)
    x = row[None, :]
    tuned = (f_strong, f_weak, f_strong + 300.0, f_weak, f_strong, f_weak - 200.0)
    steps = np.array([msdr.nco_step(f) for f in tuned], U64)
    phases = rng.integers(0, 1 << 32, ch, dtype=U64)
    modes = np.array([AM, AM, USB, LSB, AM, AM], np.int32)
    ti = tq = np.stack([bw_taps(2800.0)] * ch)
    si, sq = Bank(steps, phases).advance(n)
    chain = nco_chain(ctx, ch, ti, tq, steps, phases, modes)
    chain.set_input_rows(np.zeros(ch, np.uint32), 1)
    bank = M.BankQ15(orc, x, None, si, sq, modes, ti, tq, rows=[0] * ch)
    gains, agc_on = (4.0, 1.0, 20.0, 0.5, 2.0, 37.5), (1, 1, 1, 1, 0, 0)
    gained(chain, bank, gains, agc_on)
    drive(ctx, chain, bank, x, B, tag="trajectory")
    seen = set()
    for rx in bank.rx:
        for tag in rx.branches:
            seen.update(tag)
    assert "dropped" in seen and "up" in seen and any(s.startswith("down") for s in seen), seen
    assert bank.rx[1].val > 1.0 and "down50" in {t for tag in bank.rx[0].branches for t in tag}          # the weak station was turned up, the strong one down
    assert [rx.steps for rx in bank.rx] == [calls] * 4 + [0, 0] and bank.rx[4].val == np.float32(2.0)
    assert bank.rx[0].idx == 25 - (calls - 26)
    chain.close()


# ------------------------------------------------------------------------------------------------ 5. set_gain(1) alone
@pytest.mark.parametrize("D", [1, 4])
def test_gain_on_with_nothing_else_set_changes_no_bit(ctx, golden, D):
    rng = np.random.default_rng(9500 + D)
    ch, n = 7, 256 * D
    modes, ti, tq = mixed_bank(golden, ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=U64)
    x = levels(rng, ch, n, weak=(3,))
    outs = []
    for on in (False, True):
        chain = nco_chain(ctx, ch, ti, tq, steps, phases, modes)
        chain.set_decimation(D)
        assert chain.gain() is False
        if on:
            chain.set_gain(True)
            assert chain.gain() is True
        pitch = pitch_of(n // D)
        buf, met = ctx.to_device(np.zeros((ch, pitch, 2), I16)), ctx.to_device(np.zeros(ch, U64))
        chain.set_iq_out(buf, pitch)
        chain.set_meter(met)
        dy = ctx.array((ch, n // D), I16)
        chain.process(ctx.to_device(x), dy, n)
        outs.append((dy.download(), buf.download(), met.download()))
        if on:
            w = chain.agc_state(0)
            assert w["multiplier"] == 65536 and w["agc_idx"] == 25 and w["AGC_val"] == 1.0 and w["steps"] == 0 and w["absmax"] > 0 and not w["agc_buffer"].any()
        chain.close()
    for a, b in zip(*outs):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ 6. meter and I/Q output
def test_the_meter_is_ungained_the_pairs_are_gained_and_an_iq_only_call_steps(ctx, orc, golden):
    rng = np.random.default_rng(9600)
    ch, n = 4, 4 * B
    modes, ti, tq = mixed_bank(golden, ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=U64)
    si, sq = Bank(steps, phases).advance(n)
    x = levels(rng, ch, n, weak=())
    chain = nco_chain(ctx, ch, ti, tq, steps, phases, modes)
    bank = M.BankQ15(orc, x, None, si, sq, modes, ti, tq)
    plain = M.BankQ15(orc, x, None, si, sq, modes, ti, tq)
    gained(chain, bank, GAINS[:4], (1, 1, 1, 1))          # 0, -2.5, 0.25, 40
    meters = drive(ctx, chain, bank, x, B, iq=True, meter=True, tag="metered", span=(0, 2 * B))
    for k in range(2):          # the ungained oracle sum, whatever the gains were
        assert np.array_equal(meters[k], plain.call(k * B, (k + 1) * B, gain_on=False)[2])
    before = [rx.steps for rx in bank.rx]
    # an I/Q-only call: no audio batch; the pairs are the gained ones and the AGC steps all the same
    pitch = pitch_of(B)
    buf = ctx.to_device(np.zeros((ch, pitch, 2), I16))
    chain.set_iq_out(buf, pitch)
    chain.set_meter(None)
    chain.process(ctx.to_device(np.ascontiguousarray(x[:, 2 * B:3 * B])), None, B)
    _, pairs, _ = bank.call(2 * B, 3 * B)
    assert np.array_equal(buf.download()[:, :B], pairs)
    M.check_words(chain, bank.rx, "behind the I/Q-only call")
    assert [rx.steps for rx in bank.rx] == [s + 1 for s in before]
    # LSB / USB audio stays I -+ Q of the stored pairs
    dy = ctx.array((ch, B), I16)
    chain.process(ctx.to_device(np.ascontiguousarray(x[:, 3 * B:])), dy, B)
    want, pairs, _ = bank.call(3 * B, 4 * B)
    got, p = dy.download(), buf.download()[:, :B].astype(np.int32)
    assert np.array_equal(got, want) and np.array_equal(p, pairs)
    assert np.array_equal(got[1], (p[1, :, 0] - p[1, :, 1]).astype(I16)) and np.array_equal(got[2], (p[2, :, 0] + p[2, :, 1]).astype(I16))
    chain.close()


# ------------------------------------------------------------------------------------------------ 7. complex input
@pytest.mark.parametrize("D", [1, 3])
def test_complex_input_dir_0(ctx, orc, golden, D):
    rng = np.random.default_rng(9700 + D)
    ch, n = 5, 256 * D
    modes, ti, tq = mixed_bank(golden, ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=U64)
    si, sq = Bank(steps, phases).advance(n)
    xi, xq = levels(rng, ch, n, weak=(1,)), levels(rng, ch, n, weak=(1,))
    chain = nco_chain(ctx, ch, ti, tq, steps, phases, modes)
    chain.set_complex_input(True, 0)
    chain.set_decimation(D)
    bank = M.BankQ15(orc, xi, xq, si, sq, modes, ti, tq, direction=0)
    gained(chain, bank, GAINS[1:], (1, 0, 1, 0, 1))
    drive(ctx, chain, bank, interleave(xi, xq), 128 * D, D, iq=True, meter=True, tag="complex D %d" % D)
    chain.close()


# ------------------------------------------------------------------------------------------------ 8. the PLL and the LMS filter behind the gained pair
def test_syncam_pll_and_lms_behind_the_gain(ctx, orc, golden):
    """D = 1, MSDR_CHAIN_SYNCAM_PLL: receiver 0 (SYNCAM) hands the GAINED I and Q to the PLL demodulator; receiver 2's audio goes through the LMS filter"""
    rng = np.random.default_rng(9800)
    ch, n = 3, 3 * B
    _, ti, tq = mixed_bank(golden, ch)
    modes = np.array([SYNCAM, AM, USB], np.int32)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=U64)
    si, sq = Bank(steps, phases).advance(n)
    x = levels(rng, ch, n, weak=(0,))
    chain = nco_chain(ctx, ch, ti, tq, steps, phases, modes, flags=msdr.CHAIN_SYNCAM_PLL)
    anr_on = np.array([0, 0, 1], np.int32)
    chain.set_anr(anr_on)
    bank = M.BankQ15(orc, x, None, si, sq, modes, ti, tq)
    gained(chain, bank, (30.0, 0.5, 2.0), (1, 1, 1))
    pll, anr = orc.syncam_new(), [orc.anr_new() for _ in range(ch)]

    def post(c, audio, pairs, lo):
        if c == 0:
            audio = orc.syncam_q15(pll, np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1]))
        return orc.anr_q15(anr[c], anr_on[c], audio)
    drive(ctx, chain, bank, x, B, tag="pll + lms", post=post)
    chain.close()


# ------------------------------------------------------------------------------------------------ 9. refusals, each followed by an unchanged output
def test_refusals_change_nothing(ctx, orc, golden):
    rng = np.random.default_rng(9900)
    ch, n = 3, 4 * B
    modes, ti, tq = mixed_bank(golden, ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=U64)
    si, sq = Bank(steps, phases).advance(n)
    x = levels(rng, ch, n, weak=(1,))
    lib = ctx.lib
    # a NULL chain; a chain that is not in phase-accumulator mode
    state = np.zeros(32, np.int32)
    assert lib.msdr_chain_set_gain(None, 1) == ARG and lib.msdr_chain_set_gain_channels(None, 0, 0, None) == ARG
    assert lib.msdr_chain_set_agc(None, None, 1) == ARG and lib.msdr_chain_get_agc(None, 0, state.ctypes.data) == ARG
    table = msdr.Chain(ctx, msdr.ARITH_Q15, ch, ti[0], tq[0], mixer=msdr.MIXER_NCO, modes=modes, **any_table())
    for f, a in ((table.set_gain, (True,)), (table.set_gain_channels, (0, [1.0])), (table.set_agc, (None, 1)), (table.agc_state, (0,))):
        refused(f, *a)
    table.close()
    chain = nco_chain(ctx, ch, ti, tq, steps, phases, modes)
    refused(chain.agc_state, 0)          # no state yet
    bank = M.BankQ15(orc, x, None, si, sq, modes, ti, tq)
    gained(chain, bank, (2.0, 35.0, -1.0), (1, 1, 0))
    drive(ctx, chain, bank, x, B, tag="before", span=(0, B))
    for f, a in ((chain.set_gain_channels, (2, [1.0, 1.0])),                 # a range past `channels`
                 (chain.set_gain_channels, (4, [])),
                 (chain.set_gain_channels, (0, [1.0, float("nan")])),         # a gain that is not finite
                 (chain.set_gain_channels, (1, [float("inf")])),
                 (chain.set_agc, ([1, 2, 0],)),                               # an agc_on value other than 0 or 1
                 (chain.set_agc, ([-1, 0, 0],)),
                 (chain.set_agc, (None, 2)),
                 (chain.agc_state, (3,))):
        refused(f, *a)
        M.check_words(chain, bank.rx, "behind a refusal")
    assert lib.msdr_chain_set_gain_channels(chain.h, 0, 2, None) == ARG          # a NULL gain with count > 0
    with pytest.raises(ValueError):
        chain.set_agc([1, 1])
    drive(ctx, chain, bank, x, B, tag="behind the refusals", span=(B, 2 * B))          # (the model knows nothing of them)
    # a call that returns an error steps nothing
    with pytest.raises(msdr.MsdrError):
        chain.process(ctx.to_device(x[:, :B]), None, B)          # no audio batch and no I/Q buffer
    M.check_words(chain, bank.rx, "behind a refused call")
    # off keeps the state and runs the plain kernels; on again carries on; reset and init_fir leave the records alone
    chain.set_gain(False)
    dy = ctx.array((ch, B), I16)
    chain.process(ctx.to_device(np.ascontiguousarray(x[:, 2 * B:3 * B])), dy, B)
    assert np.array_equal(dy.download(), bank.call(2 * B, 3 * B, gain_on=False)[0])
    M.check_words(chain, bank.rx, "gain off")
    chain.set_gain(True)
    chain.process(ctx.to_device(np.ascontiguousarray(x[:, 3 * B:])), dy, B)
    assert np.array_equal(dy.download(), bank.call(3 * B, 4 * B)[0])
    M.check_words(chain, bank.rx, "on again")
    chain.reset()
    M.check_words(chain, bank.rx, "behind reset")
    chain.init_fir()
    chain.set_decimation(2)
    chain.set_decimation(1)
    M.check_words(chain, bank.rx, "behind init_fir and a neighbouring setter")
    assert chain.gain() is True
    with pytest.raises(msdr.MsdrError):
        chain.graph([ctx.to_device(x[:, :B])] * 2, [ctx.array((ch, B), I16)] * 2, B)
    chain.close()
