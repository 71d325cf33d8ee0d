"""Per-receiver decimation (Q15): msdr_chain_set_decimation(D) on a chain in phase-accumulator mode -- oscillator, FIR pair and decimator, a
bank of digital down-converters.  chain_q15pcnd_kernel mixes every input sample and evaluates the FIR pair, the demodulator and the store once
per D of them: output m of a call is what the undecimated chain's demodulator gives at input sample m * D + D - 1 (arm_fir_decimate's
convention), and the nodes behind the kernel run on that stream at fs / D.

The model is tests/test_gpu_nco_per_channel.py's: per-sample oscillator values from Bank feed orclib.Oracle.chain_q15 one channel and one
128-sample block at a time at the FULL rate, and the expected output is that stream subsampled, [D - 1::D] of every call.  Everything is int16
and bit-exact: np.array_equal, no tolerance."""
import numpy as np
import pytest

import orclib
from gpuhelp import ctx, msdr  # noqa: F401
from test_gpu_nco_per_channel import Bank, any_table, off_grid_steps, u32
from test_gpu_osc_per_channel import bw_taps, mixed_bank, oracle_row, run

pytestmark = pytest.mark.gpu
B = 128
NT = 102
FS = 24000.0
PCND = "chain_q15pcnd_kernel"
AM, LSB, USB, CW, SYNCAM = orclib.AM, orclib.LSB, orclib.USB, orclib.CW, orclib.SYNCAM
ARG, LEN = msdr.STATUS_ARGUMENT_ERROR, msdr.STATUS_LENGTH_ERROR
NOUTS = (32, 128, 256, 768)
# msdr_decpc_geometry.h at 102 taps (np = 104), 11 channels: the tile in outputs for calls of 32 / 128 / 256 / 768 outputs.  4 / 4 / 2 / 1
# channels per wave by n / D; 8 outputs per lane where four waves' windows fit 64 KB, else 4 or 2 (tests/test_decim_geometry.py holds the rule)
TILES = {2: (128, 128, 256, 512), 3: (64, 64, 256, 512), 4: (128, 128, 256, 512), 5: (64, 64, 128, 256), 8: (64, 64, 128, 256), 32: (32, 32, 64, 128)}


def decim_run(ctx, chain, x, step, D, dtype=np.int16, channels=None):
    """calls of `step` INPUT samples over x [rows, n]; d_audio is allocated as [channels, step / D]"""
    rows, n = x.shape
    ch = channels or rows
    got = np.empty((ch, n // D), dtype)
    for o in range(0, n, step):
        dx, dy = ctx.to_device(np.ascontiguousarray(x[:, o:o + step])), ctx.array((ch, step // D), dtype)
        chain.process(dx, dy, step)
        got[:, o // D:(o + step) // D] = dy.download()
    return got


def step_list(rng):
    """0, 5 * 2^25, fs / 4, -fs / 4, one LSB below zero and six seeded ones"""
    return np.concatenate([np.array([0, 5 << 25, 0x40000000, 0xC0000000, 0xFFFFFFFF], np.uint64), rng.integers(0, 1 << 32, 6, dtype=np.uint64)])


def nco_chain(ctx, ch, ti, tq, steps, phases, modes=None, **kw):
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, ti[0], tq[0], mixer=msdr.MIXER_NCO, modes=modes, **any_table(), **kw)
    chain.set_taps_channels(0, ti, tq)
    chain.set_nco_channels(0, u32(steps), u32(phases))
    return chain


# ------------------------------------------------------------------------------------------------ 1. the oracle, every geometry
@pytest.mark.parametrize("D", sorted(TILES))
def test_oracle_every_geometry(ctx, orc, golden, D):
    """11 channels (a partial group), 102 taps, AM / LSB / USB / CW; the same stream in calls of 32, 128, 256 outputs and ONE call of 768"""
    rng = np.random.default_rng(2000 + D)
    n = 768 * D
    steps = step_list(rng)
    ch = steps.size
    assert ch == 11
    modes, ti, tq = mixed_bank(golden, ch)
    phases = rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    x = rng.integers(-30000, 30001, (ch, n)).astype(np.int16)
    si, sq = Bank(steps, phases).advance(n)
    outs = []
    for nout, tile in zip(NOUTS, TILES[D]):
        chain = nco_chain(ctx, ch, ti, tq, steps, phases, modes)
        assert chain.decimation() == 1
        chain.set_decimation(D)
        assert chain.decimation() == D
        outs.append(decim_run(ctx, chain, x, nout * D, D))
        info = chain.info()
        assert info["kernel"].startswith(PCND) and info["tile"] == tile, (nout, info)
        bank = Bank(steps, phases)
        bank.advance(n)
        bank.check(chain, nout)                                          # the chain's time moved by the INPUT samples
        chain.close()
    for c in range(ch):
        want = oracle_row(orc, x[c], si[c], sq[c], lambda b: (modes[c], ti[c], tq[c]), {})[D - 1::D]
        assert want.size == 768 and np.abs(want.astype(np.int32)).max() > 100
        assert np.array_equal(outs[0][c], want), c
    for o in outs[1:]:
        assert np.array_equal(outs[0], o)


# ------------------------------------------------------------------------------------------------ 2. the undecimated twin
def test_twin_at_four(ctx, golden):
    rng = np.random.default_rng(2102)
    ch, D, n = 7, 4, 3 * 512
    modes, ti, tq = mixed_bank(golden, ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    x = rng.integers(-30000, 30001, (ch, n)).astype(np.int16)
    a, twin = nco_chain(ctx, ch, ti, tq, steps, phases, modes), nco_chain(ctx, ch, ti, tq, steps, phases, modes)
    a.set_decimation(D)
    got, full = decim_run(ctx, a, x, 512, D), run(ctx, twin, x, 512)
    assert np.array_equal(got, full[:, 3::4])
    assert a.info()["kernel"].startswith(PCND) and twin.info()["kernel"].startswith("chain_q15pcn_kernel")
    a.close()
    twin.close()


# ------------------------------------------------------------------------------------------------ 3. nothing written past the row
def guarded_call(ctx, chain, x, D, ch, dtype, sentinel):
    """one call into a batch with guard rows in front and behind and n - n / D samples of slack per row behind it, all `sentinel`;
    -> (the batch [ch, n / D], whether every other element still holds the sentinel)"""
    n = x.shape[1]
    nout = n // D
    guard, total = 2 * nout + 8, ch * nout
    flat = np.full(guard + total + ch * (n - nout) + guard, sentinel, dtype)
    buf = ctx.to_device(flat)
    chain.process(ctx.to_device(np.ascontiguousarray(x)), buf.offset(guard * flat.itemsize), n)
    back = buf.download()
    return back[guard:guard + total].reshape(ch, nout), bool((back[:guard] == sentinel).all() and (back[guard + total:] == sentinel).all())


@pytest.mark.parametrize("D", [3, 4])
def test_nothing_is_written_past_the_row(ctx, golden, D):
    rng = np.random.default_rng(2103 + D)
    ch = 11
    modes, ti, tq = mixed_bank(golden, ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    a, control = nco_chain(ctx, ch, ti, tq, steps, phases, modes), nco_chain(ctx, ch, ti, tq, steps, phases, modes)
    for o in (a, control):
        o.set_decimation(D)
    for nout in (32, 768):
        x = rng.integers(-30000, 30001, (ch, nout * D)).astype(np.int16)
        got, intact = guarded_call(ctx, a, x, D, ch, np.int16, -32768)          # (-32768: no demodulator output of this input)
        assert intact, nout
        assert np.array_equal(got, decim_run(ctx, control, x, nout * D, D)), nout
        assert (got != -32768).all()
    a.close()
    control.close()


# ------------------------------------------------------------------------------------------------ 4. the nodes at the decimated rate
def test_nodes_at_the_decimated_rate(ctx, orc):
    """two one-stage nodes per channel, designed for fs / D: a low-pass and a notch of the channel's own"""
    rng = np.random.default_rng(2104)
    ch, D, ticks = 6, 4, 6
    n = ticks * B * D
    taps = np.stack([bw_taps(900.0 + 250.0 * c) for c in range(ch)])
    lp = msdr.biquad_design(msdr.BQ_LOWPASS, 2200.0, 0.54, fs=FS / D)
    notches = np.stack([msdr.biquad_design(msdr.BQ_NOTCH, 700.0 + 90.5 * c, 12.0, fs=FS / D) for c in range(ch)])
    steps = np.array([msdr.nco_step(6000.0 + 7.3 * c) for c in range(ch)], np.uint64)
    phases = rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    chain = nco_chain(ctx, ch, taps, taps, steps, phases, mode=AM, biquad_nodes=[[lp], [notches[0]]])
    chain.set_node_coefficients_channels(1, 0, 0, notches)
    chain.set_decimation(D)
    t = np.arange(n)
    x = np.stack([(9000 * (1 + 0.5 * np.sin(2 * np.pi * (300 + 150 * c) * t / FS)) * np.cos(2 * np.pi * 6000 * t / FS + c) + rng.integers(-300, 301, n)).astype(np.int16)
                  for c in range(ch)])
    got = decim_run(ctx, chain, x, B * D, D)
    assert chain.info()["kernel"].startswith(PCND)
    assert chain.node_kernel() == "biquad_teensy_pc_kernel<2>"
    si, sq = Bank(steps, phases).advance(n)
    for c in range(ch):
        audio = oracle_row(orc, x[c], si[c], sq[c], lambda b: (AM, taps[c], taps[c]), {})[D - 1::D]
        pre = audio.copy()
        nodes = [orc.biquad_teensy_new([lp]), orc.biquad_teensy_new([notches[c]])]
        for k in range(ticks):                                           # AudioFilterBiquad::update() per tick of 128 outputs
            blk = audio[k * B:(k + 1) * B]
            for nd in nodes:
                blk = orc.biquad_teensy_update(nd, blk)
            audio[k * B:(k + 1) * B] = blk
        assert not np.array_equal(audio, pre)
        assert np.array_equal(got[c], audio), c
    chain.close()


# ------------------------------------------------------------------------------------------------ 5. live
LIVE_PLAN = [(1, 128), (1, 128), (8, 1024), (8, 1024), (3, 192), "retune", (3, 192), "retune with phases", (8, 1024), (8, 1024), (3, 384), (1, 128)]


def live_stream(ctx, rng, chain, bank, x, dtype):
    """LIVE_PLAN over a chain whose channels all hear row 0 of x: (D, input samples) per call, set_decimation between stretches with no reset,
    two retunes inside one history length (500 taps).  -> (got [ch, outputs], the INPUT index of every output, si, sq per input sample)"""
    ch = bank.step.size
    n = x.shape[1]
    si, sq = np.empty((ch, n), np.int16), np.empty((ch, n), np.int16)
    got, index, o = [], [], 0
    for item in LIVE_PLAN:
        if isinstance(item, str):
            first, count = (1, 3) if item == "retune" else (0, 3)
            ns = off_grid_steps(rng, count)
            nph = rng.integers(0, 1 << 32, count, dtype=np.uint64) if item.endswith("phases") else None
            chain.set_nco_channels(first, u32(ns), None if nph is None else u32(nph))
            bank.retune(first, ns, nph)
            bank.check(chain, item)
            continue
        D, m = item
        if chain.decimation() != D:
            chain.set_decimation(D)
        assert chain.decimation() == D
        dx, dy = ctx.to_device(np.ascontiguousarray(x[:, o:o + m])), ctx.array((ch, m // D), dtype)
        chain.process(dx, dy, m)
        got.append(dy.download())
        kernel = chain.info()["kernel"]
        assert ("pcnd_kernel" in kernel) == (D > 1), (item, kernel)
        index.append(o + D - 1 + D * np.arange(m // D))
        si[:, o:o + m], sq[:, o:o + m] = bank.advance(m)
        bank.check(chain, item)                                          # chain.nco(c) follows the model after every call
        o += m
    assert o == n
    return np.concatenate(got, axis=1), np.concatenate(index), si, sq


LIVE_N = sum(item[1] for item in LIVE_PLAN if not isinstance(item, str))


def test_live_switches_retunes_and_a_shared_row(ctx, orc):
    rng = np.random.default_rng(2105)
    ch, nt = 6, 500
    assert LIVE_N % B == 0
    taps = np.stack([bw_taps(600.0 + 300.0 * c, nt) for c in range(ch)])
    modes = np.array([(AM, LSB, USB, AM)[c % 4] for c in range(ch)], np.int32)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, taps[0], taps[0], mixer=msdr.MIXER_NCO, modes=modes, **any_table())
    chain.set_input_rows(np.zeros(ch, np.int64), 1)
    chain.set_nco_channels(0, u32(steps), u32(phases))
    chain.set_taps_channels(0, taps)
    x = rng.integers(-30000, 30001, (1, LIVE_N)).astype(np.int16)
    got, index, si, sq = live_stream(ctx, rng, chain, Bank(steps, phases), x, np.int16)
    for c in range(ch):
        want = oracle_row(orc, x[0], si[c], sq[c], lambda b: (modes[c], taps[c], taps[c]), {})
        assert np.array_equal(got[c], want[index]), c
    chain.close()


# ------------------------------------------------------------------------------------------------ 6. refusals leave the chain untouched
def test_refusals_leave_the_chain_untouched(ctx):
    rng = np.random.default_rng(2106)
    ch, D = 6, 4
    taps = np.stack([bw_taps(1200.0 + 200.0 * c) for c in range(ch)])
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    x = rng.integers(-20000, 20001, (ch, 2 * B * D)).astype(np.int16)
    lp = msdr.biquad_design(msdr.BQ_LOWPASS, 2200.0, 0.54, fs=FS / D)

    def refused(f, status):
        with pytest.raises(msdr.MsdrError) as e:
            f()
        assert e.value.status == status, e.value
        text = ctx.lib.msdr_last_error().decode()
        assert text and text in str(e.value), text

    def same(a, b, tag, d=D):
        ga, gb = decim_run(ctx, a, x, B * d, d), decim_run(ctx, b, x, B * d, d)
        assert np.array_equal(ga, gb), tag
        assert a.info() == b.info() and a.decimation() == b.decimation() == d, tag
        assert np.abs(ga.astype(np.int32)).max() > 100

    def pair(**kw):
        return [nco_chain(ctx, ch, taps, taps, steps, phases, mode=AM, **kw) for _ in range(2)]

    def process(chain, n, nout):
        chain.process(ctx.to_device(np.ascontiguousarray(x[:, :n])), ctx.array((ch, nout), np.int16), n)

    opened = []
    # n % D != 0: nothing enqueued, no state moved
    a, control = pair()
    opened += [a, control]
    for o in (a, control):
        o.set_decimation(D)
    refused(lambda: process(a, 130, 33), LEN)
    same(a, control, "n % D")
    # D = 0, D above the maximum, a factor whose window does not fit beside 102 taps (D = 59: 80 taps)
    for bad in (0, msdr.MAX_DECIMATION_Q15 + 1, 1000, 59):
        refused(lambda: a.set_decimation(bad), ARG)
    same(a, control, "bad factors")
    a.set_decimation(58)                                                 # (the largest factor at 102 taps)
    a.set_decimation(D)
    # while D > 1: set_anr with a channel on
    refused(lambda: a.set_anr(np.array([0, 1, 0, 0, 0, 0], np.int32)), ARG)
    refused(lambda: a.set_anr(None, 1), ARG)
    same(a, control, "set_anr")
    # an odd n / D with nodes
    b, b_control = pair(biquad_nodes=[[lp], [lp]])
    opened += [b, b_control]
    for o in (b, b_control):
        o.set_decimation(D)
    refused(lambda: process(b, 132, 33), LEN)
    same(b, b_control, "odd n / D with nodes")
    # an LMS channel on, then the setter
    lms, lms_control = pair()
    opened += [lms, lms_control]
    for o in (lms, lms_control):
        o.set_anr(np.array([0, 0, 1, 0, 0, 0], np.int32))
    refused(lambda: lms.set_decimation(D), ARG)
    same(lms, lms_control, "lms", 1)
    # a chain created with MSDR_CHAIN_SYNCAM_PLL
    pll, pll_control = pair(flags=msdr.CHAIN_SYNCAM_PLL)
    opened += [pll, pll_control]
    refused(lambda: pll.set_decimation(D), ARG)
    same(pll, pll_control, "pll", 1)
    # chains that are not in phase-accumulator mode: the table mixer (shared table, per-channel taps) and Fs/4
    tabs = [msdr.Chain(ctx, msdr.ARITH_Q15, ch, taps[0], taps[0], mixer=msdr.MIXER_NCO, mode=AM, **any_table()) for _ in range(2)]
    fs4s = [msdr.Chain(ctx, msdr.ARITH_Q15, ch, taps[0], taps[0], mode=AM) for _ in range(2)]
    opened += tabs + fs4s
    for o in tabs:
        o.set_taps_channels(0, taps)
    for pr in (tabs, fs4s):
        refused(lambda: pr[0].set_decimation(D), ARG)
        refused(lambda: pr[0].set_decimation(1), ARG)
        same(pr[0], pr[1], "not an NCO chain", 1)
        assert "pcnd" not in pr[0].info()["kernel"]
    # graphs stay refused; the block switch is accepted and such calls run the unfused launches
    refused(lambda: a.graph([ctx.array((ch, B * D), np.int16) for _ in range(2)], [ctx.array((ch, B), np.int16) for _ in range(2)], B * D), ARG)
    a.set_block_kernel_q15(True)
    same(a, control, "block switch")
    assert a.info()["kernel"].startswith(PCND)
    for o in opened:
        o.close()
