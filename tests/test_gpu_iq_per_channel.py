"""Baseband I/Q output of the per-receiver down-converter bank (Q15): msdr_chain_set_iq_out makes the phase-accumulator kernels store the pair
behind the channel filter -- the fi / fq their demodulator receives -- for every output, two int16 per pair, rows of `pitch` pairs in a device
buffer of the caller's.

The expected value is always orclib.Oracle.chain_q15(..., want_iq=True): pair m of a call is the oracle's full-rate (i, q) at the call's
input sample m D + D - 1, compared with ==.  The buffer is filled with a sentinel before every call, pitch = n_out rounded up to 8, plus 8:
pairs < n_out equal the oracle's, everything else is still the sentinel, and the audio is the oracle's, so the tap disturbed nothing.  The
models of the oscillators are those of tests/test_gpu_nco_per_channel.py / test_gpu_decim_per_channel.py."""
import numpy as np
import pytest

import orclib
from gpuhelp import ctx, msdr  # noqa: F401
from test_gpu_decim_per_channel import NOUTS, TILES, nco_chain, step_list
from test_gpu_nco_per_channel import Bank, any_table, off_grid_steps, u32
from test_gpu_osc_per_channel import bw_taps, lowpass, mixed_bank, notch, oracle_row

pytestmark = pytest.mark.gpu
B = 128
AM, LSB, USB, CW, SYNCAM = orclib.AM, orclib.LSB, orclib.USB, orclib.CW, orclib.SYNCAM
ARG, LEN = msdr.STATUS_ARGUMENT_ERROR, msdr.STATUS_LENGTH_ERROR
SENT = {np.dtype(np.int16): 0x5A5B, np.dtype(np.float32): 0x7B5A5B5C}          # as bit patterns; the float is 1.13e36, no FIR output


def pitch_of(n_out):
    return (n_out + 7) // 8 * 8 + 8


def sentinel(shape, dtype):
    dt = np.dtype(dtype)
    return np.full(shape, SENT[dt], np.uint16 if dt.itemsize == 2 else np.uint32).view(dt)


def bits(a):
    return a.view(np.uint16 if a.dtype.itemsize == 2 else np.uint32)


def tapped(ctx, chain, x, step, D=1, ch=None, adtype=np.int16, pdtype=np.int16, audio_of=lambda k: True):
    """set an I/Q buffer, then calls of `step` INPUT samples over x [rows, n] -> (audio [ch, n / D], pairs [ch, n / D, 2]); the rows' pitch is
    pitch_of(the longest call); before every call buffer and audio are sentinels, behind it everything past the call's n_out pairs still is.
    audio_of(k) False: call k is an I/Q-only call (d_audio None), its stretch of the audio stays sentinel."""
    n = x.shape[1]
    ch = ch or x.shape[0]
    pitch = pitch_of(min(step, n) // D)
    fresh = sentinel((ch, pitch, 2), pdtype)
    buf = ctx.to_device(fresh)
    chain.set_iq_out(buf, pitch)
    assert chain.iq_out() == (buf.ptr, pitch)
    audio, pairs = sentinel((ch, n // D), adtype).copy(), np.empty((ch, n // D, 2), pdtype)
    for k, o in enumerate(range(0, n, step)):
        m = min(step, n - o)
        buf.upload(fresh)
        dx = ctx.to_device(np.ascontiguousarray(x[:, o:o + m]))
        dy = ctx.to_device(sentinel((ch, m // D), adtype)) if audio_of(k) else None
        chain.process(dx, dy, m)
        if dy is not None:
            audio[:, o // D:(o + m) // D] = dy.download()
        back = buf.download()
        assert np.array_equal(bits(back[:, m // D:]), bits(fresh[:, m // D:])), (k, "pairs past n_out were written")
        pairs[:, o // D:(o + m) // D] = back[:, :m // D]
    return audio, pairs


def iq_of(want_row, n, step, D=1):
    """the oracle's pairs [n / D, 2] of calls of `step` input samples over the first n: (i, q) at the full rate, outputs at D - 1 + k D of a call"""
    _, i, q = want_row
    idx = np.concatenate([np.arange(lo + D - 1, min(lo + step, n), D) for lo in range(0, n, step)])
    return np.stack([i[idx], q[idx]], axis=1)


def padded(x, n128=None):
    n = x.shape[-1]
    n128 = n128 or (n + B - 1) // B * B
    return np.concatenate([x, np.zeros(x.shape[:-1] + (n128 - n,), x.dtype)], axis=-1)


def bank5(golden, ch):
    """mixed_bank with a SYNCAM channel among the AM ones (no PLL: the envelope)"""
    modes, ti, tq = mixed_bank(golden, ch)
    modes[4::8] = SYNCAM
    return modes, ti, tq


# ------------------------------------------------------------------------------------------------ 1. every sliding-window geometry
def test_every_sliding_window_geometry(ctx, orc, golden):
    """10 channels (a partial group at 4 and at 2 channels per wave), 102 taps, AM / LSB / USB / CW / SYNCAM, off-grid steps; 768 samples as
    6 calls of 128, 3 of 256, one of 768 (tiles 128 / 256 / 512): the same pairs"""
    rng = np.random.default_rng(5100)
    ch, n = 10, 6 * B
    modes, ti, tq = bank5(golden, ch)
    assert set(modes.tolist()) == {AM, LSB, USB, CW, SYNCAM}
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    si, sq = Bank(steps, phases).advance(n)
    x = rng.integers(-30000, 30001, (ch, n)).astype(np.int16)
    want = [oracle_row(orc, x[c], si[c], sq[c], lambda b: (modes[c], ti[c], tq[c]), {}, want_iq=True) for c in range(ch)]
    runs = []
    for step, tile in ((B, 128), (2 * B, 256), (n, 512)):
        chain = nco_chain(ctx, ch, ti, tq, steps, phases, modes)
        audio, pairs = tapped(ctx, chain, x, step)
        info = chain.info()
        assert info["kernel"].startswith("chain_q15pcn_kernel") and info["tile"] == tile, info          # the names stay
        for c in range(ch):
            assert np.array_equal(audio[c], want[c][0]), (step, c)
            assert np.array_equal(pairs[c], iq_of(want[c], n, step)), (step, c)
        assert np.abs(pairs.astype(np.int32)).max() > 1000
        runs.append(pairs)
        chain.close()
    assert np.array_equal(runs[0], runs[1]) and np.array_equal(runs[0], runs[2])


# ------------------------------------------------------------------------------------------------ 2. the tail and the segments
@pytest.mark.parametrize("n", [1001, 4600])
def test_the_tail_and_the_segments(ctx, orc, golden, n):
    """3 channels, one call.  1001: tile 512, the second tile partly live, the last live lane holding 1 of its 8 pairs.  4600: two time segments."""
    rng = np.random.default_rng(5200 + n)
    ch = 3
    n128 = (n + B - 1) // B * B
    modes, ti, tq = mixed_bank(golden, ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    si, sq = Bank(steps, phases).advance(n128)
    x = rng.integers(-30000, 30001, (ch, n)).astype(np.int16)
    chain = nco_chain(ctx, ch, ti, tq, steps, phases, modes)
    audio, pairs = tapped(ctx, chain, x, n)
    info = chain.info()
    assert info["tile"] == 512 and (info["time_segments"] >= 2) == (n == 4600), info
    for c in range(ch):
        want = oracle_row(orc, padded(x[c]), si[c], sq[c], lambda b: (modes[c], ti[c], tq[c]), {}, want_iq=True)
        assert np.array_equal(audio[c], want[0][:n]), c
        assert np.array_equal(pairs[c], iq_of(want, n, n)), c
    chain.close()


# ------------------------------------------------------------------------------------------------ 3. decimation
@pytest.fixture(scope="module")
def dec_ref(orc, golden):
    """one full-rate reference for every factor: 11 channels (step_list), mixed modes, 1001 * 32 samples and the rest of the last block"""
    rng = np.random.default_rng(5300)
    steps = step_list(rng)
    ch = steps.size
    modes, ti, tq = mixed_bank(golden, ch)
    phases = rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    n128 = (1001 * 32 + B - 1) // B * B
    x = rng.integers(-30000, 30001, (ch, n128)).astype(np.int16)
    si, sq = Bank(steps, phases).advance(n128)
    want = [oracle_row(orc, x[c], si[c], sq[c], lambda b: (modes[c], ti[c], tq[c]), {}, want_iq=True) for c in range(ch)]
    return dict(steps=steps, phases=phases, modes=modes, ti=ti, tq=tq, x=x, want=want, ch=ch)


@pytest.mark.parametrize("D", [2, 3, 8, 32])
def test_decimation(ctx, dec_ref, D):
    """the factors and lengths of tests/test_gpu_decim_per_channel.py: 768 D inputs in calls of 32, 128, 256 and 768 outputs (both copy
    layouts, every read width, 2 / 4 / 8 outputs per lane) and one call of 1001 outputs for the tail; pair m is the full-rate (i, q)[m D + D - 1]"""
    r = dec_ref
    for nout, tile in tuple(zip(NOUTS, TILES[D])) + ((1001, None),):
        chain = nco_chain(ctx, r["ch"], r["ti"], r["tq"], r["steps"], r["phases"], r["modes"])
        chain.set_decimation(D)
        m = (1001 if nout == 1001 else 768) * D
        audio, pairs = tapped(ctx, chain, r["x"][:, :m], nout * D, D)
        info = chain.info()
        assert info["kernel"].startswith("chain_q15pcnd_kernel") and (tile is None or info["tile"] == tile), (nout, info)
        for c in range(r["ch"]):
            assert np.array_equal(audio[c], r["want"][c][0][D - 1:m:D]), (nout, c)
            assert np.array_equal(pairs[c], iq_of(r["want"][c], m, nout * D, D)), (nout, c)
        chain.close()


def test_the_factor_switched_between_calls(ctx, dec_ref):
    r = dec_ref
    ch, want = r["ch"], r["want"]
    chain = nco_chain(ctx, ch, r["ti"], r["tq"], r["steps"], r["phases"], r["modes"])
    pitch = pitch_of(128)
    fresh = sentinel((ch, pitch, 2), np.int16)
    buf = ctx.to_device(fresh)
    chain.set_iq_out(buf, pitch)
    lo = 0
    for D, m in ((2, 256), (8, 1024), (1, 128), (3, 384)):
        if D != chain.decimation():
            chain.set_decimation(D)
        assert chain.iq_out() == (buf.ptr, pitch)
        buf.upload(fresh)
        dy = ctx.array((ch, m // D), np.int16)
        chain.process(ctx.to_device(np.ascontiguousarray(r["x"][:, lo:lo + m])), dy, m)
        back, audio = buf.download(), dy.download()
        assert np.array_equal(back[:, m // D:], fresh[:, m // D:]), D
        for c in range(ch):
            idx = np.arange(lo + D - 1, lo + m, D)
            assert np.array_equal(audio[c], want[c][0][idx]), (D, c)
            assert np.array_equal(back[c, :m // D], np.stack([want[c][1][idx], want[c][2][idx]], axis=1)), (D, c)
        lo += m
    chain.close()


# ------------------------------------------------------------------------------------------------ 4. saturation
def test_saturated_pairs(ctx, orc):
    """sin = cos = -23170; the two newest samples times 32767 each: pair 0 is (-23170, -23170), pairs 1 .. 255 saturate at (-32768, -32768)"""
    ch, n, nt = 2, 256, 102
    steps, phases = np.zeros(ch, np.uint64), np.full(ch, 0xA0000000, np.uint64)
    s, c = msdr.nco_q15(u32(phases))
    assert s.tolist() == [-23170] * ch and c.tolist() == [-23170] * ch
    taps = np.zeros((ch, nt), np.int16)
    taps[:, -2:] = 32767
    x = np.full((ch, n), 32767, np.int16)
    chain = nco_chain(ctx, ch, taps, taps, steps, phases, mode=AM)
    _, pairs = tapped(ctx, chain, x, n)
    si, sq = Bank(steps, phases).advance(n)
    for k in range(ch):
        want = oracle_row(orc, x[k], si[k], sq[k], lambda b: (AM, taps[k], taps[k]), {}, want_iq=True)
        assert (want[1][0], want[2][0]) == (-23170, -23170) and (want[1][1:] == -32768).all() and (want[2][1:] == -32768).all()
        assert np.array_equal(pairs[k], iq_of(want, n, n)), k
        assert pairs[k, 0].tolist() == [-23170, -23170] and (pairs[k, 1:] == -32768).all()
    chain.close()


# ------------------------------------------------------------------------------------------------ 5. with the meter
@pytest.mark.parametrize("D, n_out", [(1, 4600), (8, 2100)])
@pytest.mark.parametrize("order", ["meter first", "iq first"])
def test_beside_the_meter(ctx, orc, golden, D, n_out, order):
    """both set, one call in two or more time segments: the meter is the oracle's sum and the sum of squares of the downloaded pairs"""
    rng = np.random.default_rng(5500 + D)
    ch, n = 3, n_out * D
    n128 = (n + B - 1) // B * B
    modes, ti, tq = mixed_bank(golden, ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    si, sq = Bank(steps, phases).advance(n128)
    x = rng.integers(-30000, 30001, (ch, n)).astype(np.int16)
    chain = nco_chain(ctx, ch, ti, tq, steps, phases, modes)
    if D > 1:
        chain.set_decimation(D)
    meter = ctx.array((ch,), np.uint64).fill(0xA5)
    if order == "meter first":
        chain.set_meter(meter)
    else:
        chain.set_iq_out(ctx.array((ch, 8, 2), np.int16), 8)          # (replaced by tapped()'s buffer: the meter is set while a buffer is)
        chain.set_meter(meter)
    audio, pairs = tapped(ctx, chain, x, n, D)
    got = meter.download()
    info = chain.info()
    assert info["time_segments"] >= 2 and info["kernel"].startswith("chain_q15pcnd_kernel" if D > 1 else "chain_q15pcn_kernel"), info
    assert chain.meter() == meter.ptr
    for c in range(ch):
        want = oracle_row(orc, padded(x[c]), si[c], sq[c], lambda b: (modes[c], ti[c], tq[c]), {}, want_iq=True)
        wp = iq_of(want, n, n, D)
        assert np.array_equal(audio[c], want[0][D - 1:n:D]), c
        assert np.array_equal(pairs[c], wp), c
        assert int(got[c]) == int((wp.astype(np.int64) ** 2).sum()) == int((pairs[c].astype(np.int64) ** 2).sum()), c
    chain.close()


# ------------------------------------------------------------------------------------------------ 6. shared input
@pytest.mark.parametrize("n_inputs", [1, 3])
def test_receivers_on_shared_antenna_rows(ctx, orc, golden, n_inputs):
    rng = np.random.default_rng(5600 + n_inputs)
    ch, n = 7, 3 * B
    modes, ti, tq = mixed_bank(golden, ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    rows = (np.arange(ch) * 2) % n_inputs
    chain = nco_chain(ctx, ch, ti, tq, steps, phases, modes)
    chain.set_input_rows(rows.astype(np.int64), n_inputs)
    x = rng.integers(-30000, 30001, (n_inputs, n)).astype(np.int16)
    audio, pairs = tapped(ctx, chain, x, B, ch=ch)
    si, sq = Bank(steps, phases).advance(n)
    for c in range(ch):
        want = oracle_row(orc, x[rows[c]], si[c], sq[c], lambda b: (modes[c], ti[c], tq[c]), {}, want_iq=True)
        assert np.array_equal(audio[c], want[0]), c
        assert np.array_equal(pairs[c], iq_of(want, n, B)), c
    chain.close()


# ------------------------------------------------------------------------------------------------ 7. I/Q-only calls
def test_iq_only_calls_leave_the_nodes_alone(ctx, orc):
    """two one-stage nodes; calls 0, 2, 4 have no audio batch: pairs exact on every call, the audio of calls 1, 3, 5 is the oracle's demodulator
    output of those blocks through nodes that never saw the others"""
    rng = np.random.default_rng(5700)
    ch, ticks = 5, 6
    n = ticks * B
    taps = np.stack([bw_taps(1500.0 + 300.0 * c) for c in range(ch)])
    modes = np.array([AM, USB, LSB, AM, USB], np.int32)
    notches = np.stack([notch(c) for c in range(ch)])
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    chain = nco_chain(ctx, ch, taps, taps, steps, phases, modes, biquad_nodes=[[lowpass()], [notches[0]]])
    chain.set_node_coefficients_channels(1, 0, 0, notches)
    x = rng.integers(-20000, 20001, (ch, n)).astype(np.int16)
    with pytest.raises(msdr.MsdrError) as e:                            # no buffer: a null audio batch stays refused
        chain.process(ctx.to_device(np.ascontiguousarray(x[:, :B])), None, B)
    assert e.value.status == ARG
    audio, pairs = tapped(ctx, chain, x, B, audio_of=lambda k: k % 2 == 1)
    si, sq = Bank(steps, phases).advance(n)
    for c in range(ch):
        want = oracle_row(orc, x[c], si[c], sq[c], lambda b: (modes[c], taps[c], taps[c]), {}, want_iq=True)
        assert np.array_equal(pairs[c], iq_of(want, n, B)), c
        nodes = [orc.biquad_teensy_new([lowpass()]), orc.biquad_teensy_new([notches[c]])]
        for k in range(ticks):
            blk = want[0][k * B:(k + 1) * B]
            if k % 2 == 0:
                assert (bits(audio[c, k * B:(k + 1) * B]) == SENT[np.dtype(np.int16)]).all(), (c, k)
                continue
            for nd in nodes:
                blk = orc.biquad_teensy_update(nd, blk)
            assert np.array_equal(audio[c, k * B:(k + 1) * B], blk), (c, k)
    chain.set_iq_out(None)
    with pytest.raises(msdr.MsdrError) as e:
        chain.process(ctx.to_device(np.ascontiguousarray(x[:, :B])), None, B)
    assert e.value.status == ARG
    chain.close()


# ------------------------------------------------------------------------------------------------ 8. the contract
def call(ctx, chain, x, D=1):
    dy = ctx.array((x.shape[0], x.shape[1] // D), np.int16)
    chain.process(ctx.to_device(np.ascontiguousarray(x)), dy, x.shape[1])
    return dy.download()


def test_refusals_lengths_off_and_what_the_setting_survives(ctx, orc):
    rng = np.random.default_rng(5800)
    ch, n = 5, 6 * B
    taps = np.stack([bw_taps(1200.0 + 300.0 * c) for c in range(ch)])
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    x = rng.integers(-30000, 30001, (ch, n)).astype(np.int16)
    si, sq = Bank(steps, phases).advance(n)
    want = [oracle_row(orc, x[c], si[c], sq[c], lambda b: (USB, taps[c], taps[c]), {}, want_iq=True) for c in range(ch)]
    w_audio = np.stack([w[0] for w in want])
    w_pairs = np.stack([np.stack([w[1], w[2]], axis=1) for w in want])          # [ch, n, 2]
    pitch = pitch_of(B)
    fresh = sentinel((ch, pitch, 2), np.int16)
    first, second = ctx.to_device(fresh), ctx.to_device(fresh)

    def block(k, buf, chain):
        """call k of the stream: the audio and the pairs are the oracle's, the rest of buf is untouched"""
        buf.upload(fresh)
        assert np.array_equal(call(ctx, chain, x[:, k * B:(k + 1) * B]), w_audio[:, k * B:(k + 1) * B]), k
        back = buf.download()
        assert np.array_equal(back[:, :B], w_pairs[:, k * B:(k + 1) * B]) and np.array_equal(back[:, B:], fresh[:, B:]), k

    # a chain that never called set_nco_channels refuses, and so does a null chain (tests/test_iq_abi.py)
    plain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, taps[0], taps[0], mixer=msdr.MIXER_NCO, mode=USB, **any_table())
    plain.set_taps_channels(0, taps)
    for args in ((first, pitch), (None, 0)):
        with pytest.raises(msdr.MsdrError) as e:
            plain.set_iq_out(*args)
        assert e.value.status == ARG
    assert plain.iq_out() == (None, 0)
    plain.close()

    chain = nco_chain(ctx, ch, taps, taps, steps, phases, mode=USB)
    assert chain.iq_out() == (None, 0)
    chain.set_iq_out(first, pitch)
    block(0, first, chain)
    # every refusal leaves the setting and the next call alone
    for args in ((second.offset(8), pitch), (second.offset(4), pitch), (second, 0), (second, pitch - 4), (second, 12)):
        with pytest.raises(msdr.MsdrError) as e:
            chain.set_iq_out(*args)
        assert e.value.status == ARG and chain.iq_out() == (first.ptr, pitch), args[1]
    block(1, first, chain)
    assert np.array_equal(bits(second.download()), bits(fresh))
    # n_out > pitch: nothing enqueued, no state moved -- the stream continues bit-exactly
    first.upload(fresh)
    with pytest.raises(msdr.MsdrError) as e:
        call(ctx, chain, x[:, 2 * B:2 * B + pitch + 8])
    assert e.value.status == LEN and np.array_equal(bits(first.download()), bits(fresh))
    block(2, first, chain)
    # off: the same kernel name, nothing written; on again, another buffer
    chain.set_iq_out(None)
    assert chain.iq_out() == (None, 0)
    first.upload(fresh)
    assert np.array_equal(call(ctx, chain, x[:, 3 * B:4 * B]), w_audio[:, 3 * B:4 * B])
    assert np.array_equal(bits(first.download()), bits(fresh)) and chain.info()["kernel"].startswith("chain_q15pcn_kernel")
    chain.set_iq_out(second, pitch)
    block(4, second, chain)
    assert np.array_equal(bits(first.download()), bits(fresh))
    # the setting survives set_meter, a retune, set_taps_channels, init_fir and reset
    meter = ctx.array((ch,), np.uint64).fill(0)
    chain.set_meter(meter)
    assert chain.iq_out() == (second.ptr, pitch)
    block(5, second, chain)
    assert np.array_equal(meter.download(), (w_pairs[:, 5 * B:].astype(np.int64) ** 2).sum(axis=(1, 2)).astype(np.uint64))
    chain.set_meter(None)
    chain.init_fir()
    assert chain.iq_out() == (second.ptr, pitch)
    chain.reset()
    chain.set_taps_channels(0, taps)
    chain.set_nco_channels(0, u32(steps), u32(phases))
    assert chain.iq_out() == (second.ptr, pitch)
    block(0, second, chain)                                              # from a clear history again
    chain.close()
