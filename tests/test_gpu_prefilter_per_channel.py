"""Two-stage decimation for the Q15 down-converter bank: msdr_chain_set_prefilter(D1, taps) puts one chain-wide real filter that decimates by
D1 in front of every receiver's channel pair, which runs at fs / D1 and decimates by msdr_chain_set_decimation's D2; chain_q15pcn2_kernel
keeps raw IF history only and recomputes the intermediates a tile shares with the one before it.

The expected value is composed from the oracle's own stages (tests/prefilter_model.py: freqconv_q15 over the Bank's oscillator rows, the
prefilter through arm_fir_fast_q15, [D1 - 1 :: D1], the channel pair through arm_fir_fast_q15, [D2 - 1 :: D2], the demodulator).  Everything is
int16 and bit-exact: np.array_equal, no tolerance, whatever the split into calls, tiles, chunks and time segments."""
import ctypes as C

import numpy as np
import pytest

import orclib
import prefilter_model as pm
from gpuhelp import ctx, msdr  # noqa: F401
from test_gpu_decim_per_channel import decim_run, guarded_call, nco_chain
from test_gpu_nco_per_channel import Bank, off_grid_steps, u32
from test_gpu_osc_per_channel import bw_taps, mixed_bank

pytestmark = pytest.mark.gpu
PCN2 = "chain_q15pcn2_kernel"
AM, LSB, USB, CW = orclib.AM, orclib.LSB, orclib.USB, orclib.CW
I16 = np.int16


def pre_chain(ctx, ch, ti, tq, steps, phases, modes, p, D1, D2, **kw):
    chain = nco_chain(ctx, ch, ti, tq, steps, phases, modes=modes, **kw)
    chain.set_prefilter(D1, p)
    if D2 > 1:
        chain.set_decimation(D2)
    assert chain.prefilter() == (D1, p.size) and chain.decimation() == D2
    return chain


def model(orc, x, si, sq, p, D1, modes, ti, tq, D2):
    """audio [ch, n / (D1 D2)] of the whole stream"""
    return np.stack([pm.model_q15(orc, x[c], si[c], sq[c], p, D1, modes[c], ti[c], tq[c], D2)[0] for c in range(len(modes))])


# ------------------------------------------------------------------------------------------------ 1. the oracle, every geometry and call split
@pytest.mark.parametrize("shape", pm.SHAPES)
def test_oracle_every_geometry(ctx, orc, golden, shape):
    """11 channels (a partial group), 102 taps, AM / LSB / USB / CW; the same stream in calls of 32, 128, 256 outputs and ONE call of 768"""
    D1, N1, D2 = shape
    rng = np.random.default_rng([3000, D1, N1, D2])
    steps = pm.step_list(rng)
    ch, n = steps.size, 768 * D1 * D2
    assert ch == pm.CH
    modes, ti, tq = mixed_bank(golden, ch)
    phases = rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    p = pm.lowpass(D1, N1, I16)
    x = rng.integers(-30000, 30001, (ch, n)).astype(I16)
    si, sq = Bank(steps, phases).advance(n)
    want = model(orc, x, si, sq, p, D1, modes, ti, tq, D2)
    assert np.abs(want.astype(np.int32)).max() > 1000
    outs = []
    for nout, tile in zip(pm.NOUTS, pm.TILES["q15"][shape]):
        chain = pre_chain(ctx, ch, ti, tq, steps, phases, modes, p, D1, D2)
        outs.append(decim_run(ctx, chain, x, nout * D1 * D2, D1 * D2))
        info = chain.info()
        assert info["kernel"].startswith(PCN2) and info["tile"] == tile and info["taps_padded"] == 104, (nout, info)
        g = pm.geometry(False, pm.pad(N1, False), D1, 104, D2, nout, ch, 256)
        assert info["lds_bytes"] == g["lds_bytes"] and info["block"] == g["block"], (nout, info, g)
        chain.close()
    for k, got in enumerate(outs):
        bad = np.argwhere(got != want)
        assert bad.size == 0, (shape, pm.NOUTS[k], bad[:4], len(bad))
    for got in outs[1:]:
        assert np.array_equal(got, outs[0])


def test_one_call_in_time_segments(ctx, orc, golden):
    """(4, 16, 4), one call of 4096 outputs: two time segments of four tiles, each starting from raw samples alone"""
    D1, N1, D2 = pm.SEGMENTED["shape"]
    rng = np.random.default_rng(3001)
    steps = pm.step_list(rng)
    ch, n = steps.size, pm.SEGMENTED["nout"] * D1 * D2
    modes, ti, tq = mixed_bank(golden, ch)
    phases = rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    p = pm.lowpass(D1, N1, I16)
    x = rng.integers(-30000, 30001, (ch, n)).astype(I16)
    si, sq = Bank(steps, phases).advance(n)
    chain = pre_chain(ctx, ch, ti, tq, steps, phases, modes, p, D1, D2)
    got = decim_run(ctx, chain, x, n, D1 * D2)
    info = chain.info()
    assert info["kernel"].startswith(PCN2) and info["tile"] == pm.SEGMENTED["tile"]["q15"] and info["time_segments"] == pm.SEGMENTED["nseg"]["q15"] >= 2, info
    assert np.array_equal(got, model(orc, x, si, sq, p, D1, modes, ti, tq, D2))
    chain.close()


# ------------------------------------------------------------------------------------------------ 2. guards
def test_nothing_is_written_past_the_rows_of_audio_and_pairs(ctx, orc, golden):
    D1, N1, D2 = 4, 16, 4
    rng = np.random.default_rng(3002)
    ch = 11
    modes, ti, tq = mixed_bank(golden, ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    p = pm.lowpass(D1, N1, I16)
    for nout in (32, 200):
        x = rng.integers(-30000, 30001, (ch, nout * D1 * D2)).astype(I16)
        a = pre_chain(ctx, ch, ti, tq, steps, phases, modes, p, D1, D2)
        pitch = (nout + 7) // 8 * 8 + 8
        buf = ctx.to_device(np.full((ch + 2) * pitch * 2, -77, I16))          # pairs: a guard row in front and behind, the slack of every row
        a.set_iq_out(buf.offset(pitch * 4), pitch)
        got, intact = guarded_call(ctx, a, x, D1 * D2, ch, I16, I16(-32768))
        assert intact, nout
        pairs = buf.download().reshape(ch + 2, pitch, 2)
        assert (pairs[0] == -77).all() and (pairs[-1] == -77).all() and (pairs[1:-1, nout:] == -77).all(), nout
        si, sq = Bank(steps, phases).advance(x.shape[1])
        for c in range(ch):
            audio, fi, fq = pm.model_q15(orc, x[c], si[c], sq[c], p, D1, modes[c], ti[c], tq[c], D2)
            assert np.array_equal(got[c], audio) and np.array_equal(pairs[1 + c, :nout, 0], fi) and np.array_equal(pairs[1 + c, :nout, 1], fq), (nout, c)
        a.close()


# ------------------------------------------------------------------------------------------------ 3. live changes between calls
def test_a_retune_and_a_tap_change_between_calls(ctx, orc):
    """6 AM / LSB channels at (8, 32, 4); calls of 64 outputs: behind call 2 channels 1 .. 3 are retuned phase-continuously, behind call 4
    channels 2 .. 4 get other channel taps (the pCoeffs rewrite of a stage-2 instance: its state, the intermediates, stays)"""
    D1, N1, D2 = 8, 32, 4
    rng = np.random.default_rng(3003)
    ch, calls, nout = 6, 6, 64
    step = nout * D1 * D2
    n = calls * step
    modes = np.array([AM, LSB, AM, USB, AM, LSB], np.int32)
    t0 = np.stack([bw_taps(600.0 + 500.0 * c) for c in range(ch)])
    t1 = np.stack([bw_taps(2900.0 - 300.0 * c) for c in range(ch)])
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    new_steps = off_grid_steps(rng, 3)
    p = pm.lowpass(D1, N1, I16)
    x = rng.integers(-30000, 30001, (ch, n)).astype(I16)
    chain = pre_chain(ctx, ch, t0, t0, steps, phases, modes, p, D1, D2)
    bank = Bank(steps, phases)
    got, si, sq = [], [], []
    for k in range(calls):
        if k == 2:
            chain.set_nco_channels(1, u32(new_steps))
            bank.retune(1, new_steps)
        if k == 4:
            chain.set_taps_channels(2, t1[2:5], t1[2:5])
        got.append(decim_run(ctx, chain, x[:, k * step:(k + 1) * step], step, D1 * D2))
        a, b = bank.advance(step)
        si.append(a)
        sq.append(b)
        bank.check(chain, k)
    got, si, sq = np.concatenate(got, 1), np.concatenate(si, 1), np.concatenate(sq, 1)
    assert chain.info()["kernel"].startswith(PCN2)
    for c in range(ch):
        want = pm.model_q15(orc, x[c], si[c], sq[c], p, D1, modes[c], t0[c], t0[c], D2)[0]
        if 2 <= c < 5:
            late = pm.model_q15(orc, x[c], si[c], sq[c], p, D1, modes[c], t1[c], t1[c], D2)[0]
            want = np.concatenate([want[:4 * nout], late[4 * nout:]])
        assert np.array_equal(got[c], want), c
    chain.close()


def test_reset_and_init_fir(ctx, orc, golden):
    D1, N1, D2 = 4, 16, 4
    rng = np.random.default_rng(3004)
    ch, nout = 5, 96
    n = nout * D1 * D2
    modes, ti, tq = mixed_bank(golden, ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    p = pm.lowpass(D1, N1, I16)
    x = rng.integers(-30000, 30001, (ch, 3 * n)).astype(I16)
    chain = pre_chain(ctx, ch, ti, tq, steps, phases, modes, p, D1, D2)
    bank = Bank(steps, phases)
    parts = []
    for k in range(3):
        if k == 1:
            chain.init_fir()          # the FIR history alone: the oscillators carry on
        if k == 2:
            chain.reset()             # ... and time and phases too
            bank.reset()
        got = decim_run(ctx, chain, x[:, k * n:(k + 1) * n], n // 2, D1 * D2)
        si, sq = bank.advance(n)
        parts.append((got, model(orc, x[:, k * n:(k + 1) * n], si, sq, p, D1, modes, ti, tq, D2)))
        assert chain.prefilter() == (D1, N1) and chain.decimation() == D2
    for k, (got, want) in enumerate(parts):
        assert np.array_equal(got, want), k
    # a clear history is where the row may change: another prefilter directly after init_fir
    chain.init_fir()
    p2 = pm.lowpass(D1, 30, I16)
    chain.set_prefilter(D1, p2)
    got = decim_run(ctx, chain, x[:, :n], n, D1 * D2)
    si, sq = bank.advance(n)
    assert np.array_equal(got, model(orc, x[:, :n], si, sq, p2, D1, modes, ti, tq, D2))
    chain.close()


def test_set_decimation_switched_between_calls(ctx, orc, golden):
    """D2 4 -> 3 -> 1 -> 4 behind calls of 96 D1 12 samples: the channel pair's output at fs / D1 is one stream, picked every D2-th"""
    D1, N1 = 4, 16
    rng = np.random.default_rng(3005)
    ch, inter = 5, 96 * 12          # intermediates per call: a multiple of every D2
    step = inter * D1
    seq = (4, 3, 1, 4)
    n = len(seq) * step
    modes, ti, tq = mixed_bank(golden, ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    p = pm.lowpass(D1, N1, I16)
    x = rng.integers(-30000, 30001, (ch, n)).astype(I16)
    si, sq = Bank(steps, phases).advance(n)
    chain = pre_chain(ctx, ch, ti, tq, steps, phases, modes, p, D1, 1)
    for k, D2 in enumerate(seq):
        chain.set_decimation(D2)
        got = decim_run(ctx, chain, x[:, k * step:(k + 1) * step], step, D1 * D2)
        assert chain.info()["kernel"].startswith(PCN2)
        for c in range(ch):
            _, fi, fq = pm.model_q15(orc, x[c], si[c], sq[c], p, D1, modes[c], ti[c], tq[c], 1)
            pick = np.arange(k * inter + D2 - 1, (k + 1) * inter, D2)
            assert np.array_equal(got[c], orc.demod_q15(int(modes[c]), fi[pick], fq[pick])), (k, D2, c)
    chain.close()


# ------------------------------------------------------------------------------------------------ 4. one antenna row
@pytest.mark.parametrize("ch", [1, 5, 17])
def test_a_shared_antenna_row(ctx, orc, golden, ch):
    D1, N1, D2 = 8, 32, 4
    rng = np.random.default_rng(3006 + ch)
    nout = 160
    n = nout * D1 * D2
    modes, ti, tq = mixed_bank(golden, ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    p = pm.lowpass(D1, N1, I16)
    x = rng.integers(-30000, 30001, (1, n)).astype(I16)
    si, sq = Bank(steps, phases).advance(n)
    chain = pre_chain(ctx, ch, ti, tq, steps, phases, modes, p, D1, D2)
    chain.set_input_rows(np.zeros(ch, np.int64), 1)
    got = decim_run(ctx, chain, x, n // 2, D1 * D2, channels=ch)
    assert chain.info()["kernel"].startswith(PCN2)
    assert np.array_equal(got, model(orc, np.repeat(x, ch, 0), si, sq, p, D1, modes, ti, tq, D2))
    chain.close()


# ------------------------------------------------------------------------------------------------ 5. the edges of stage 1's arithmetic
def test_stage_one_saturates_and_wraps_as_arm_fir_fast_q15_does(ctx, orc):
    """full-scale rows (constant, alternating, random signs) at step 0 -- the mixer passes them at 32767 / 32768 -- through a prefilter whose
    sum of magnitudes is far above 32768: intermediates that saturate at both rails and accumulators that wrap"""
    D1, D2 = 4, 2
    rng = np.random.default_rng(3007)
    ch, nout = 4, 128
    n = nout * D1 * D2
    p = np.array([30000, -30000] * 8, I16)          # sum |p| = 480 000: |acc| reaches 1.5e10 >> 2^31
    p2 = np.full(16, 12000, I16)                    # sum = 192 000: saturates, and wraps at full scale
    t = np.stack([bw_taps(1500.0 + 400.0 * c) for c in range(ch)])
    modes = np.array([LSB, USB, AM, LSB], np.int32)
    x = np.stack([np.full(n, 32767, I16), np.where(np.arange(n) & 1, -32768, 32767).astype(I16),
                  rng.choice(np.array([-32768, 32767], I16), n), rng.integers(-32768, 32768, n).astype(I16)])
    steps, phases = np.zeros(ch, np.uint64), np.zeros(ch, np.uint64)          # cos = 32767, sin = 0
    seen = dict(high=False, low=False, wrap=False)
    for row in (p, p2):
        si, sq = Bank(steps, phases).advance(n)
        chain = pre_chain(ctx, ch, t, t, steps, phases, modes, row, D1, D2)
        pitch = nout + 8
        buf = ctx.to_device(np.zeros((ch, pitch, 2), I16))
        chain.set_iq_out(buf, pitch)
        got = decim_run(ctx, chain, x, n, D1 * D2)
        pairs = buf.download()
        for c in range(ch):
            mi, _ = orc.freqconv_q15(x[c], np.zeros_like(x[c]), si[c], sq[c], 1, 1)
            rc, u = orc.fir_q15_blocks(row, mi, 128)
            assert rc == 0
            true = np.convolve(mi.astype(np.int64), row[::-1].astype(np.int64))[:n]          # the accumulators before they wrap
            seen["high"] |= bool((u == 32767).any())
            seen["low"] |= bool((u == -32768).any())
            seen["wrap"] |= bool((np.abs(true) >= 1 << 31).any())
            audio, fi, fq = pm.model_q15(orc, x[c], si[c], sq[c], row, D1, modes[c], t[c], t[c], D2)
            assert np.array_equal(got[c], audio) and np.array_equal(pairs[c, :nout, 0], fi) and np.array_equal(pairs[c, :nout, 1], fq), c
        chain.close()
    assert all(seen.values()), ("the case must reach both rails and wrap an accumulator", seen)


# ------------------------------------------------------------------------------------------------ 6. refusals: nothing changed
def test_every_refusal_leaves_the_chain_as_it_was(ctx, orc, golden):
    D1, N1, D2 = 4, 16, 4
    rng = np.random.default_rng(3008)
    ch, nout = 5, 64
    n = nout * D1 * D2
    modes, ti, tq = mixed_bank(golden, ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    p = pm.lowpass(D1, N1, I16)
    x = rng.integers(-30000, 30001, (ch, 2 * n)).astype(I16)
    si, sq = Bank(steps, phases).advance(2 * n)
    want = model(orc, x, si, sq, p, D1, modes, ti, tq, D2)
    lib = ctx.lib

    def refused(f, *a):
        with pytest.raises(msdr.MsdrError) as e:
            f(*a)
        assert e.value.status == msdr.STATUS_ARGUMENT_ERROR, e.value
        assert "nothing changed" in str(e.value) or "nothing enqueued" in str(e.value), e.value

    # a chain that is not in phase-accumulator mode
    from test_gpu_nco_per_channel import any_table
    plain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, ti[0], tq[0], mixer=msdr.MIXER_NCO, modes=modes, **any_table())
    refused(plain.set_prefilter, D1, p)
    assert plain.prefilter() == (1, 0)
    plain.close()

    chain = nco_chain(ctx, ch, ti, tq, steps, phases, modes=modes)
    pf = p.astype(np.float32)
    assert lib.msdr_chain_set_prefilter_f32(chain.h, C.c_uint32(D1), C.c_uint32(N1), pf.ctypes.data_as(C.c_void_p)) == msdr.STATUS_ARGUMENT_ERROR          # the other arithmetic's
    assert lib.msdr_chain_set_prefilter(chain.h, C.c_uint32(D1), C.c_uint32(N1), None) == msdr.STATUS_ARGUMENT_ERROR                                      # a NULL row
    for bad in (0, 3, 6, 64):
        if bad:
            refused(chain.set_prefilter, bad, p)
    refused(chain.set_prefilter, D1, p[:15])          # an odd count
    refused(chain.set_prefilter, 32, np.ones(40000, I16))          # no geometry fits
    chain.set_complex_input(1, 0)
    refused(chain.set_prefilter, D1, p)               # complex input on
    chain.set_complex_input(0)
    assert chain.prefilter() == (1, 0)
    chain.set_prefilter(D1, p)
    refused(chain.set_complex_input, 1, 0)            # ... and the other way round
    chain.set_decimation(D2)
    refused(chain.set_decimation, 57)                 # fits the one-stage kernel (1024 D + 12 np <= 61 440), not beside the stage-1 chunk
    assert chain.decimation() == D2
    chain.set_block_kernel_q15(1)                     # accepted: such calls run the unfused launches
    with pytest.raises(msdr.MsdrError):
        msdr.ChainGraph(chain, [ctx.array((ch, 128), I16)] * 2, [ctx.array((ch, 8), I16)] * 2, 128)          # graphs stay refused

    dx, dy = ctx.to_device(x[:, :n + 8]), ctx.array((ch, nout + 1), I16)
    with pytest.raises(msdr.MsdrError) as e:
        chain.process(dx, dy, n + 8)                  # a multiple of D1 and of D2, not of D1 * D2
    assert e.value.status == msdr.STATUS_LENGTH_ERROR
    got = [decim_run(ctx, chain, x[:, :n], n, D1 * D2)]
    # the history is no longer clear: the row stays what it is
    refused(chain.set_prefilter, D1, pm.lowpass(D1, 30, I16))
    refused(chain.set_prefilter, 8, p)
    refused(chain.set_prefilter, 1, p)                # turning it off needs a clear history too
    refused(chain.set_prefilter, D1, None)
    assert chain.prefilter() == (D1, N1)
    got.append(decim_run(ctx, chain, x[:, n:], n, D1 * D2))
    assert chain.info()["kernel"].startswith(PCN2)
    assert np.array_equal(np.concatenate(got, 1), want)
    # off over a clear history: the one-stage kernel again, and on again
    chain.reset()
    chain.set_prefilter(1, None)
    assert chain.prefilter() == (1, 0)
    decim_run(ctx, chain, x[:, :n], n, D2)
    assert chain.info()["kernel"].startswith("chain_q15pcnd_kernel")
    chain.close()
