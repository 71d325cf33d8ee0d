"""Baseband I/Q output of the per-receiver down-converter bank (F32): msdr_chain_set_iq_out on fp32 chains -- two floats per pair, the two fp32
FIR sums in in_scale units, from the IQ flavours of chain_f32pcn / chain_f32pcnd.

Reference.  The oracle exposes no fp32 I and Q, but its demodulator is I + Q in mode USB and I - Q in mode LSB: per channel,
orclib.Oracle.chain_f32 with that channel's taps and oscillator and no cascade in both modes, and in float64 I = (usb + lsb) / 2,
Q = (usb - lsb) / 2 (exact up to the two roundings of the reference's own add and subtract, near 1e-7).
Condition, per channel over a run: sqrt(sum |dI|^2 + |dQ|^2) / sqrt(sum I^2 + Q^2) < 1e-5.  It is the chain's own clause: e_go < 1e-5 on both
audio rows I + Q and I - Q gives exactly this bound on the pair (|d(I+Q)|^2 + |d(I-Q)|^2 = 2 (|dI|^2 + |dQ|^2), and the same for the
references' energies).  Every case prints its ratio; about 5e-7 is expected.
Three conditions with teeth beside it: on chains without a cascade and with float output the audio of USB / LSB channels IS
np.float32(I) +/- np.float32(Q) of the downloaded pairs, bit for bit (pf_demod's own statement: a swapped or negated pair fails); audio and
meter with the tap on are bit-identical to a twin chain with it off; two fresh chains give identical pairs."""
import numpy as np
import pytest

import orclib
from f32pc_cases import B, bw_taps
from gpuhelp import ctx, msdr  # noqa: F401
from test_gpu_decim_per_channel import NOUTS, step_list
from test_gpu_decim_per_channel_f32 import TILES, nco_chain
from test_gpu_iq_per_channel import bits, pitch_of, sentinel, tapped
from test_gpu_nco_per_channel import Bank, off_grid_steps, u32
from test_gpu_nco_per_channel_f32 import any_table, f32
from test_gpu_osc_per_channel_f32 import mixed_bank, signal

pytestmark = pytest.mark.gpu
AM, LSB, USB, CW = orclib.AM, orclib.LSB, orclib.USB, orclib.CW
ARG, LEN = msdr.STATUS_ARGUMENT_ERROR, msdr.STATUS_LENGTH_ERROR
F = np.float32


def iq_ref(orc, x, ti, tq, si, sq):
    """(I, Q) float64 at the full rate from the oracle's USB and LSB audio of one channel"""
    usb = orc.chain_f32(x, USB, ti, tq, si, sq, None).astype(np.float64)
    lsb = orc.chain_f32(x, LSB, ti, tq, si, sq, None).astype(np.float64)
    return (usb + lsb) / 2, (usb - lsb) / 2


def out_index(n, step, D=1):
    return np.concatenate([np.arange(lo + D - 1, min(lo + step, n), D) for lo in range(0, n, step)])


def judged(tag, pairs, ref, idx):
    """pairs [m, 2] of one channel against the reference at the inputs idx"""
    i, q = ref[0][idx], ref[1][idx]
    p = pairs.astype(np.float64)
    ratio = float(np.sqrt(((p[:, 0] - i) ** 2 + (p[:, 1] - q) ** 2).sum()) / np.sqrt((i * i + q * q).sum()))
    print("iq %s ratio %.3e" % (tag, ratio))
    assert ratio < 1e-5, (tag, ratio)


def ssb_is_the_pairs(audio, pairs, modes):
    """pf_demod's statement on float audio without a cascade: USB = I + Q, LSB = I - Q in fp32"""
    seen = 0
    for c, m in enumerate(modes):
        if m in (USB, LSB):
            want = pairs[c, :, 0] + pairs[c, :, 1] if m == USB else pairs[c, :, 0] - pairs[c, :, 1]
            assert want.dtype == F and np.array_equal(bits(want), bits(audio[c])), c
            seen += 1
    assert seen


def plain_run(ctx, chain, x, step, D=1, ch=None):
    """the same calls without a tap -> audio [ch, n / D]"""
    n = x.shape[1]
    ch = ch or x.shape[0]
    audio = np.empty((ch, n // D), F)
    for o in range(0, n, step):
        m = min(step, n - o)
        dy = ctx.array((ch, m // D), F)
        chain.process(ctx.to_device(np.ascontiguousarray(x[:, o:o + m])), dy, m)
        audio[:, o // D:(o + m) // D] = dy.download()
    return audio


def ftapped(ctx, chain, x, step, D=1, ch=None):
    return tapped(ctx, chain, x, step, D, ch=ch, adtype=F, pdtype=F)


# ------------------------------------------------------------------------------------------------ 1. every sliding-window geometry
def test_every_sliding_window_geometry(ctx, orc):
    rng = np.random.default_rng(6100)
    ch, n = 10, 6 * B
    modes, ti, tq = mixed_bank(ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    si, sq = (f32(v) for v in Bank(steps, phases).advance(n))
    x = signal(rng, ch, n)
    ref = [iq_ref(orc, x[c], ti[c], tq[c], si[c], sq[c]) for c in range(ch)]
    runs = []
    for step, tile in ((B, 128), (2 * B, 256), (n, 512)):
        a, b, off = (nco_chain(ctx, ch, ti, tq, steps, phases, modes=modes) for _ in range(3))
        audio, pairs = ftapped(ctx, a, x, step)
        _, again = ftapped(ctx, b, x, step)
        plain = plain_run(ctx, off, x, step)
        info = a.info()
        assert info["kernel"].startswith("chain_f32pcn_kernel") and info["tile"] == tile and info["flavour"] & msdr.FLAVOUR_IQ_OUT, info
        assert not off.info()["flavour"] & msdr.FLAVOUR_IQ_OUT and info["flavour"] == off.info()["flavour"] | msdr.FLAVOUR_IQ_OUT
        assert np.array_equal(bits(pairs), bits(again)), step          # two fresh chains, the same calls: the same bits
        assert np.array_equal(bits(audio), bits(plain)), step          # the tap disturbed nothing
        ssb_is_the_pairs(audio, pairs, modes)
        for c in range(ch):
            judged("step %d ch %d" % (step, c), pairs[c], ref[c], out_index(n, step))
        runs.append(pairs)
        a.set_iq_out(None)                                             # the flavour bit exactly while a buffer is set
        a.process(ctx.to_device(np.ascontiguousarray(x[:, :B])), ctx.array((ch, B), F), B)
        assert not a.info()["flavour"] & msdr.FLAVOUR_IQ_OUT and a.info()["kernel"].startswith("chain_f32pcn_kernel")
        for o in (a, b, off):
            o.close()
    assert np.array_equal(bits(runs[0]), bits(runs[1])) and np.array_equal(bits(runs[0]), bits(runs[2]))          # (a lane's sums do not depend on the tile)


# ------------------------------------------------------------------------------------------------ 2. the tail and the segments
@pytest.mark.parametrize("n, segs", [(1001, 0), (4600, 0), (4600, 3)])
def test_the_tail_and_the_segments(ctx, orc, n, segs):
    rng = np.random.default_rng(6200 + n + segs)
    ch = 3
    modes, ti, tq = mixed_bank(ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    si, sq = (f32(v) for v in Bank(steps, phases).advance(n))
    x = signal(rng, ch, n)
    a, off = (nco_chain(ctx, ch, ti, tq, steps, phases, modes=modes, time_segments=segs) for _ in range(2))
    audio, pairs = ftapped(ctx, a, x, n)
    info = a.info()
    assert info["tile"] == 512 and info["time_segments"] == (1 if n == 1001 else segs or 2), info
    assert np.array_equal(bits(audio), bits(plain_run(ctx, off, x, n)))
    ssb_is_the_pairs(audio, pairs, modes)
    for c in range(ch):
        judged("n %d segs %d ch %d" % (n, segs, c), pairs[c], iq_ref(orc, x[c], ti[c], tq[c], si[c], sq[c]), np.arange(n))
    a.close()
    off.close()


# ------------------------------------------------------------------------------------------------ 3. decimation
@pytest.fixture(scope="module")
def dec_ref(orc):
    """one full-rate reference for every factor: 11 channels (step_list), mixed modes, 1001 * 32 samples"""
    rng = np.random.default_rng(6300)
    steps = step_list(rng)
    ch = steps.size
    modes, ti, tq = mixed_bank(ch)
    phases = rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    n = 1001 * 32
    x = signal(rng, ch, n)
    si, sq = (f32(v) for v in Bank(steps, phases).advance(n))
    ref = [iq_ref(orc, x[c], ti[c], tq[c], si[c], sq[c]) for c in range(ch)]
    return dict(steps=steps, phases=phases, modes=modes, ti=ti, tq=tq, x=x, ref=ref, ch=ch)


@pytest.mark.parametrize("D", [2, 3, 8, 32])
def test_decimation(ctx, dec_ref, D):
    """768 D inputs in calls of 32, 128, 256 and 768 outputs (every read width, 2 / 4 / 8 outputs per lane) and one call of 1001 outputs for the tail"""
    r = dec_ref
    for nout, tile in tuple(zip(NOUTS, TILES[D])) + ((1001, None),):
        a, off = (nco_chain(ctx, r["ch"], r["ti"], r["tq"], r["steps"], r["phases"], modes=r["modes"]) for _ in range(2))
        for o in (a, off):
            o.set_decimation(D)
        m = (1001 if nout == 1001 else 768) * D
        audio, pairs = ftapped(ctx, a, r["x"][:, :m], nout * D, D)
        info = a.info()
        assert info["kernel"].startswith("chain_f32pcnd_kernel") and (tile is None or info["tile"] == tile), (nout, info)
        assert info["flavour"] & msdr.FLAVOUR_IQ_OUT and info["flavour"] & msdr.FLAVOUR_DECIMATED, info
        assert np.array_equal(bits(audio), bits(plain_run(ctx, off, r["x"][:, :m], nout * D, D))), nout
        ssb_is_the_pairs(audio, pairs, r["modes"])
        for c in range(r["ch"]):
            judged("D %d nout %d ch %d" % (D, nout, c), pairs[c], r["ref"][c], out_index(m, nout * D, D))
        a.close()
        off.close()


def test_the_factor_switched_between_calls(ctx, dec_ref):
    r = dec_ref
    ch = r["ch"]
    chain = nco_chain(ctx, ch, r["ti"], r["tq"], r["steps"], r["phases"], modes=r["modes"])
    pitch = pitch_of(128)
    fresh = sentinel((ch, pitch, 2), F)
    buf = ctx.to_device(fresh)
    chain.set_iq_out(buf, pitch)
    lo, got, idx = 0, [], []
    for D, m in ((2, 256), (8, 1024), (1, 128), (3, 384)):
        if D != chain.decimation():
            chain.set_decimation(D)
        assert chain.iq_out() == (buf.ptr, pitch)
        buf.upload(fresh)
        chain.process(ctx.to_device(np.ascontiguousarray(r["x"][:, lo:lo + m])), ctx.array((ch, m // D), F), m)
        back = buf.download()
        assert np.array_equal(bits(back[:, m // D:]), bits(fresh[:, m // D:])), D
        got.append(back[:, :m // D])
        idx.append(np.arange(lo + D - 1, lo + m, D))
        lo += m
    got, idx = np.concatenate(got, axis=1), np.concatenate(idx)
    for c in range(ch):
        judged("switched ch %d" % c, got[c], r["ref"][c], idx)
    chain.close()


# ------------------------------------------------------------------------------------------------ 5. with the meter
@pytest.mark.parametrize("D, n_out", [(1, 4600), (8, 2100)])
def test_beside_the_meter(ctx, orc, D, n_out):
    """both set, one call in two or more time segments: audio and meter are those of a twin chain with the meter alone, bit for bit; the
    meter is the sum of squares of the downloaded pairs as far as its fp32 lane sums allow (8 terms, all positive: 8 * 2^-24 of the sum)"""
    rng = np.random.default_rng(6500 + D)
    ch, n = 3, n_out * D
    modes, ti, tq = mixed_bank(ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    si, sq = (f32(v) for v in Bank(steps, phases).advance(n))
    x = signal(rng, ch, n)
    a, off = (nco_chain(ctx, ch, ti, tq, steps, phases, modes=modes) for _ in range(2))
    meters = [ctx.array((ch,), np.float64).fill(0xA5) for _ in range(2)]
    for o, mt in zip((a, off), meters):
        if D > 1:
            o.set_decimation(D)
        o.set_meter(mt)
    audio, pairs = ftapped(ctx, a, x, n, D)
    plain = plain_run(ctx, off, x, n, D)
    info = a.info()
    assert info["time_segments"] >= 2 and info["flavour"] & msdr.FLAVOUR_IQ_OUT and info["flavour"] & msdr.FLAVOUR_METER, info
    assert info["flavour"] == off.info()["flavour"] | msdr.FLAVOUR_IQ_OUT
    got, want = meters[0].download(), meters[1].download()
    assert np.array_equal(bits(audio), bits(plain)) and np.array_equal(got.view(np.uint64), want.view(np.uint64))
    ssb_is_the_pairs(audio, pairs, modes)
    for c in range(ch):
        s = float((pairs[c].astype(np.float64) ** 2).sum())
        assert s > 0 and abs(got[c] - s) <= 8 * 2.0 ** -24 * s, (c, got[c], s)
        judged("meter D %d ch %d" % (D, c), pairs[c], iq_ref(orc, x[c], ti[c], tq[c], si[c], sq[c]), np.arange(D - 1, n, D))
    a.close()
    off.close()


# ------------------------------------------------------------------------------------------------ 6. shared input
@pytest.mark.parametrize("n_inputs", [1, 3])
def test_receivers_on_shared_antenna_rows(ctx, orc, n_inputs):
    rng = np.random.default_rng(6600 + n_inputs)
    ch, n = 7, 3 * B
    modes, ti, tq = mixed_bank(ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    rows = (np.arange(ch) * 2) % n_inputs
    a, off = (nco_chain(ctx, ch, ti, tq, steps, phases, modes=modes) for _ in range(2))
    for o in (a, off):
        o.set_input_rows(rows.astype(np.int64), n_inputs)
    x = signal(rng, n_inputs, n)
    audio, pairs = ftapped(ctx, a, x, B, ch=ch)
    assert np.array_equal(bits(audio), bits(plain_run(ctx, off, x, B, ch=ch)))
    assert a.info()["flavour"] & msdr.FLAVOUR_SHARED_IF and a.info()["flavour"] & msdr.FLAVOUR_IQ_OUT
    ssb_is_the_pairs(audio, pairs, modes)
    si, sq = (f32(v) for v in Bank(steps, phases).advance(n))
    for c in range(ch):
        judged("n_inputs %d ch %d" % (n_inputs, c), pairs[c], iq_ref(orc, x[rows[c]], ti[c], tq[c], si[c], sq[c]), np.arange(n))
    a.close()
    off.close()


# ------------------------------------------------------------------------------------------------ 8. the contract
def test_refusals_lengths_off_and_what_the_setting_survives(ctx, orc):
    rng = np.random.default_rng(6800)
    ch, n = 5, 6 * B
    taps = np.stack([bw_taps(1200.0 + 300.0 * c) for c in range(ch)])
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    x = signal(rng, ch, n)
    pitch = pitch_of(B)
    fresh = sentinel((ch, pitch, 2), F)
    first, second = ctx.to_device(fresh), ctx.to_device(fresh)

    def make(**kw):
        return nco_chain(ctx, ch, taps, taps, steps, phases, mode=USB, **kw)

    # what the stream gives, from a twin with a buffer throughout: audio [ch, n] and pairs [ch, n, 2]; judged once, compared bit for bit below
    twin = make()
    w_audio, w_pairs = ftapped(ctx, twin, x, B)
    twin.close()
    si, sq = (f32(v) for v in Bank(steps, phases).advance(n))
    for c in range(ch):
        judged("contract ch %d" % c, w_pairs[c], iq_ref(orc, x[c], taps[c], taps[c], si[c], sq[c]), np.arange(n))
    ssb_is_the_pairs(w_audio, w_pairs, [USB] * ch)

    def block(k, buf, chain, dtype=F):
        buf.upload(fresh)
        dy = ctx.array((ch, B), dtype)
        chain.process(ctx.to_device(np.ascontiguousarray(x[:, k * B:(k + 1) * B])), dy, B)
        back = buf.download()
        assert np.array_equal(bits(back[:, :B]), bits(w_pairs[:, k * B:(k + 1) * B])) and np.array_equal(bits(back[:, B:]), bits(fresh[:, B:])), k
        return dy.download()

    plain = msdr.Chain(ctx, msdr.ARITH_F32, ch, taps[0], taps[0], mixer=msdr.MIXER_NCO, mode=USB, **any_table())          # no set_nco_channels
    plain.set_taps_channels_f32(0, taps)
    for args in ((first, pitch), (None, 0)):
        with pytest.raises(msdr.MsdrError) as e:
            plain.set_iq_out(*args)
        assert e.value.status == ARG
    assert plain.iq_out() == (None, 0)
    plain.close()

    chain = make()
    chain.set_iq_out(first, pitch)
    assert np.array_equal(bits(block(0, first, chain)), bits(w_audio[:, :B]))
    for args in ((second.offset(8), pitch), (second.offset(4), pitch), (second, 0), (second, pitch - 4), (second, 12)):
        with pytest.raises(msdr.MsdrError) as e:
            chain.set_iq_out(*args)
        assert e.value.status == ARG and chain.iq_out() == (first.ptr, pitch), args[1]
    assert np.array_equal(bits(block(1, first, chain)), bits(w_audio[:, B:2 * B]))
    assert np.array_equal(bits(second.download()), bits(fresh))
    first.upload(fresh)
    with pytest.raises(msdr.MsdrError) as e:                            # n_out > pitch: nothing enqueued, no state moved
        chain.process(ctx.to_device(np.ascontiguousarray(x[:, 2 * B:2 * B + pitch + 8])), ctx.array((ch, pitch + 8), F), pitch + 8)
    assert e.value.status == LEN and np.array_equal(bits(first.download()), bits(fresh))
    assert np.array_equal(bits(block(2, first, chain)), bits(w_audio[:, 2 * B:3 * B]))
    # an I/Q-only call: the pairs as always, and the stream's audio goes on behind it
    first.upload(fresh)
    chain.process(ctx.to_device(np.ascontiguousarray(x[:, 3 * B:4 * B])), None, B)
    assert np.array_equal(bits(first.download()[:, :B]), bits(w_pairs[:, 3 * B:4 * B])) and chain.info()["flavour"] & msdr.FLAVOUR_IQ_OUT
    # off: the same kernel name, the bit gone, nothing written
    chain.set_iq_out(None)
    assert chain.iq_out() == (None, 0)
    first.upload(fresh)
    dy = ctx.array((ch, B), F)
    chain.process(ctx.to_device(np.ascontiguousarray(x[:, 4 * B:5 * B])), dy, B)
    assert np.array_equal(bits(dy.download()), bits(w_audio[:, 4 * B:5 * B])) and np.array_equal(bits(first.download()), bits(fresh))
    assert chain.info()["kernel"].startswith("chain_f32pcn_kernel") and not chain.info()["flavour"] & msdr.FLAVOUR_IQ_OUT
    with pytest.raises(msdr.MsdrError) as e:                            # and a null audio batch is refused again
        chain.process(ctx.to_device(np.ascontiguousarray(x[:, 5 * B:])), None, B)
    assert e.value.status == ARG
    # the setting survives set_meter, init_fir, reset, set_taps_channels_f32 and a retune
    chain.set_iq_out(second, pitch)
    meter = ctx.array((ch,), np.float64).fill(0)
    chain.set_meter(meter)
    assert chain.iq_out() == (second.ptr, pitch)
    assert np.array_equal(bits(block(5, second, chain)), bits(w_audio[:, 5 * B:]))
    assert meter.download().min() > 0
    chain.set_meter(None)
    chain.init_fir()
    assert chain.iq_out() == (second.ptr, pitch)
    chain.reset()
    chain.set_taps_channels_f32(0, taps)
    chain.set_nco_channels(0, u32(steps), u32(phases))
    assert chain.iq_out() == (second.ptr, pitch)
    assert np.array_equal(bits(block(0, second, chain)), bits(w_audio[:, :B]))          # from a clear history again
    chain.close()
    # under MSDR_CHAIN_OUT_I16 the pairs are floats all the same: the float chain's, bit for bit
    i16 = make(flags=msdr.CHAIN_OUT_I16)
    i16.set_iq_out(first, pitch)
    a16 = block(0, first, i16, np.int16)
    assert np.abs(a16.astype(np.float64) - np.clip(np.round(w_audio[:, :B].astype(np.float64) * 32768.0), -32768, 32767)).max() <= 1
    i16.close()
