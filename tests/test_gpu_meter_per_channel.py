"""The per-receiver S-meter (Q15): msdr_chain_set_meter makes the per-receiver chain kernels sum I^2 + Q^2 of the two FIR outputs -- the fi / fq
their demodulator receives -- over every call, one uint64 per channel in a device buffer of the caller's.

The expected value is always orclib.Oracle.chain_q15(..., want_iq=True): sum(i.astype(int64) ** 2 + q.astype(int64) ** 2) over the call's
outputs, compared with ==.  The models of the oscillators are those of tests/test_gpu_osc_per_channel.py / test_gpu_nco_per_channel.py /
test_gpu_decim_per_channel.py; the audio is checked beside the meter, so the measurement did not disturb the store."""
import numpy as np
import pytest

import orclib
from gpuhelp import ctx, msdr  # noqa: F401
from test_gpu_decim_per_channel import NOUTS, TILES, nco_chain, step_list
from test_gpu_nco_per_channel import Bank, any_table, off_grid_steps, u32
from test_gpu_osc_per_channel import at, bw_taps, lowpass, mixed_bank, notch, oracle_row, rows

pytestmark = pytest.mark.gpu
B = 128
AM, LSB, USB, CW, SYNCAM = orclib.AM, orclib.LSB, orclib.USB, orclib.CW, orclib.SYNCAM
ARG, LEN = msdr.STATUS_ARGUMENT_ERROR, msdr.STATUS_LENGTH_ERROR
SENTINEL = 0xA5A5A5A5A5A5A5A5
POLICIES = ("shared table", "table per channel", "nco")


def metered(ctx, chain, x, step, D=1, ch=None, adtype=np.int16, mdtype=np.uint64):
    """set a meter, then calls of `step` INPUT samples over x [rows, n] -> (audio [ch, n / D], the meter after every call [calls, ch])"""
    n = x.shape[1]
    ch = ch or x.shape[0]
    buf = ctx.array((ch,), mdtype).fill(0xA5)
    chain.set_meter(buf)
    assert chain.meter() == buf.ptr
    audio, meters = np.empty((ch, n // D), adtype), []
    for o in range(0, n, step):
        m = min(step, n - o)
        dx, dy = ctx.to_device(np.ascontiguousarray(x[:, o:o + m])), ctx.array((ch, m // D), adtype)
        chain.process(dx, dy, m)
        audio[:, o // D:(o + m) // D] = dy.download()
        meters.append(buf.download())
    return audio, np.stack(meters)


def sums(i, q, n, step, D=1):
    """the oracle's meter of every call of `step` input samples over the first n: I and Q at the full rate, outputs at D - 1 + k D"""
    e = i.astype(np.int64) ** 2 + q.astype(np.int64) ** 2
    return np.array([int(e[lo + D - 1:min(lo + step, n):D].sum()) for lo in range(0, n, step)], np.uint64)


def padded(x, n128=None):
    n = x.shape[-1]
    n128 = n128 or (n + B - 1) // B * B
    return np.concatenate([x, np.zeros(x.shape[:-1] + (n128 - n,), x.dtype)], axis=-1)


def bank_of(ctx, policy, rng, ch, n, modes, ti, tq, **kw):
    """a chain of one oscillator policy and the per-sample oscillator values (si, sq) [ch, n] of its model"""
    if policy == "nco":
        steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
        si, sq = Bank(steps, phases).advance(n)
        return (lambda: nco_chain(ctx, ch, ti, tq, steps, phases, modes, **kw)), si, sq
    oi, oq = rows(ch, 128, seed=5)
    if policy == "shared table":
        oi, oq = np.tile(oi[:1], (ch, 1)), np.tile(oq[:1], (ch, 1))

    def make():
        chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, ti[0], tq[0], mixer=msdr.MIXER_NCO, modes=modes, osc_i=oi[0], osc_q=oq[0], **kw)
        chain.set_taps_channels(0, ti, tq)
        if policy == "table per channel":
            chain.set_osc_channels(0, oi, oq)
        return chain
    return make, at(oi, 0, n), at(oq, 0, n)


KERNEL = {"shared table": "chain_q15pc_kernel", "table per channel": "chain_q15pco_kernel", "nco": "chain_q15pcn_kernel"}


# ------------------------------------------------------------------------------------------------ 3a. every sliding-window geometry
@pytest.mark.parametrize("policy", POLICIES)
def test_every_sliding_window_geometry(ctx, orc, golden, policy):
    """10 channels (a partial group at 4 and at 2 channels per wave), 102 taps, AM / LSB / USB / CW; 6 calls of 128, 3 of 256, one of 768"""
    rng = np.random.default_rng(3100 + POLICIES.index(policy))
    ch, n = 10, 6 * B
    modes, ti, tq = mixed_bank(golden, ch)
    make, si, sq = bank_of(ctx, policy, rng, ch, n, modes, ti, tq)
    x = rng.integers(-30000, 30001, (ch, n)).astype(np.int16)
    want = [oracle_row(orc, x[c], si[c], sq[c], lambda b: (modes[c], ti[c], tq[c]), {}, want_iq=True) for c in range(ch)]
    totals = []
    for step, tile in ((B, 128), (2 * B, 256), (n, 512)):
        chain = make()
        audio, meters = metered(ctx, chain, x, step)
        info = chain.info()
        assert info["kernel"].startswith(KERNEL[policy]) and info["tile"] == tile, info          # the names of the unmetered kernels
        for c in range(ch):
            assert np.array_equal(audio[c], want[c][0]), (step, c)
            assert np.array_equal(meters[:, c], sums(want[c][1], want[c][2], n, step)), (step, c)
        assert meters.min() > 0
        totals.append(meters.sum(axis=0))
        chain.close()
    assert np.array_equal(totals[0], totals[1]) and np.array_equal(totals[0], totals[2])


# ------------------------------------------------------------------------------------------------ 3b. the tail, 3c. segments
@pytest.mark.parametrize("policy", POLICIES)
@pytest.mark.parametrize("n", [1001, 4600])
def test_the_tail_and_the_segments(ctx, orc, golden, policy, n):
    """3 channels, one call.  1001: one channel per wave, tile 512, the second tile partly live, the last live lane holding 1 of its 8 outputs.
    4600: 9 tiles in 2 segments of 5 (msdr_pc_geometry.h), the last tile slot of segment 1 empty; the partials go through the reducer."""
    rng = np.random.default_rng(3200 + n + POLICIES.index(policy))
    ch = 3
    n128 = (n + B - 1) // B * B
    modes, ti, tq = mixed_bank(golden, ch)
    make, si, sq = bank_of(ctx, policy, rng, ch, n128, modes, ti, tq)
    x = rng.integers(-30000, 30001, (ch, n)).astype(np.int16)
    chain = make()
    audio, meters = metered(ctx, chain, x, n)
    info = chain.info()
    assert info["tile"] == 512 and (info["time_segments"] >= 2) == (n == 4600), info
    for c in range(ch):
        a, i, q = oracle_row(orc, padded(x[c]), si[c], sq[c], lambda b: (modes[c], ti[c], tq[c]), {}, want_iq=True)
        assert np.array_equal(audio[c], a[:n]), c
        assert meters[0, c] == sums(i, q, n, n)[0], (c, meters[0, c])
        assert meters[0, c] != sums(i, q, n128, n128)[0]          # (the outputs past n are not nothing)
    chain.close()


# ------------------------------------------------------------------------------------------------ 3d. saturation and the 2^31 term
def test_saturation_and_the_term_of_two_to_the_31(ctx, orc):
    """sin = cos = -23170; the two newest samples times 32767 each: output 0 is (-23170, -23170), outputs 1 .. 255 saturate at (-32768, -32768)"""
    ch, n, nt = 2, 256, 102
    steps, phases = np.zeros(ch, np.uint64), np.full(ch, 0xA0000000, np.uint64)
    s, c = msdr.nco_q15(u32(phases))
    assert s.tolist() == [-23170] * ch and c.tolist() == [-23170] * ch
    taps = np.zeros((ch, nt), np.int16)
    taps[:, -2:] = 32767
    x = np.full((ch, n), 32767, np.int16)
    chain = nco_chain(ctx, ch, taps, taps, steps, phases, mode=AM)
    _, meters = metered(ctx, chain, x, n)
    si, sq = Bank(steps, phases).advance(n)
    for k in range(ch):
        _, i, q = oracle_row(orc, x[k], si[k], sq[k], lambda b: (AM, taps[k], taps[k]), {}, want_iq=True)
        assert (i[0], q[0]) == (-23170, -23170) and (i[1:] == -32768).all() and (q[1:] == -32768).all()
        assert sums(i, q, n, n)[0] == 548682028040 == 2 * 23170 ** 2 + 255 * 2 ** 31
        assert meters[0, k] == 548682028040, (k, meters[0, k])
    chain.close()


# ------------------------------------------------------------------------------------------------ 3e. decimation
@pytest.mark.parametrize("D", [3, 4, 8])
def test_decimation(ctx, orc, golden, D):
    """11 channels, 102 taps, mixed modes: 768 D inputs in calls of 32, 128, 256 outputs and one of 768 (2, 4 and 8 outputs per lane at D = 8),
    and one call of 1001 outputs for the tail; the full-rate oracle's I / Q at [D - 1::D]"""
    rng = np.random.default_rng(3500 + D)
    steps = step_list(rng)
    ch = steps.size
    modes, ti, tq = mixed_bank(golden, ch)
    phases = rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    n_tail = 1001 * D
    n128 = (n_tail + B - 1) // B * B
    x = rng.integers(-30000, 30001, (ch, n_tail)).astype(np.int16)
    si, sq = Bank(steps, phases).advance(n128)
    want = [oracle_row(orc, padded(x[c], n128), si[c], sq[c], lambda b: (modes[c], ti[c], tq[c]), {}, want_iq=True) for c in range(ch)]
    n = 768 * D
    for nout, tile in tuple(zip(NOUTS, TILES[D])) + ((1001, None),):
        chain = nco_chain(ctx, ch, ti, tq, steps, phases, modes)
        chain.set_decimation(D)
        m = n_tail if nout == 1001 else n
        audio, meters = metered(ctx, chain, x[:, :m], nout * D, D)
        info = chain.info()
        assert info["kernel"].startswith("chain_q15pcnd_kernel") and (tile is None or info["tile"] == tile), (nout, info)
        for c in range(ch):
            assert np.array_equal(audio[c], want[c][0][D - 1:m:D]), (nout, c)
            assert np.array_equal(meters[:, c], sums(want[c][1], want[c][2], m, nout * D, D)), (nout, c)
        chain.close()


# ------------------------------------------------------------------------------------------------ 3f. neighbours
def test_a_syncam_pll_chain_hands_i_and_q_on_and_is_measured_all_the_same(ctx, orc):
    rng = np.random.default_rng(3601)
    ch, n = 6, 4 * B
    t = np.arange(n)
    x = np.stack([(9000 * (1 + 0.5 * np.sin(2 * np.pi * 400 * t / 24000)) * np.cos(2 * np.pi * 6000 * t / 24000 + c) + rng.integers(-100, 101, n)).astype(np.int16)
                  for c in range(ch)])
    taps = np.stack([bw_taps(2000.0 + 400.0 * c) for c in range(ch)])
    modes = np.array([AM, SYNCAM, AM, AM, SYNCAM, SYNCAM], np.int32)
    a = 2 * np.pi * (30 + np.arange(ch))[:, None] * np.arange(B)[None, :] / B + 0.3 * np.arange(ch)[:, None]
    oi, oq = np.round(32767 * np.sin(a)).astype(np.int16), np.round(32767 * np.cos(a)).astype(np.int16)
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, taps[0], taps[0], mixer=msdr.MIXER_NCO, modes=modes, osc_i=oi[0], osc_q=oq[0], flags=msdr.CHAIN_SYNCAM_PLL)
    chain.set_osc_channels(0, oi, oq)
    chain.set_taps_channels(0, taps)
    audio, meters = metered(ctx, chain, x, B)
    si, sq = at(oi, 0, n), at(oq, 0, n)
    for c in range(ch):
        want, i, q = oracle_row(orc, x[c], si[c], sq[c], lambda b: (AM, taps[c], taps[c]), {}, want_iq=True)
        if modes[c] == SYNCAM:
            want = orc.syncam_q15(orc.syncam_new(), i, q)
        assert np.array_equal(audio[c], want), c
        assert np.array_equal(meters[:, c], sums(i, q, n, B)), c
    chain.close()


def test_nodes_per_channel_and_an_lms_channel_are_behind_the_meter(ctx, orc):
    rng = np.random.default_rng(3602)
    ch, ticks = 5, 4
    n = ticks * B
    taps = np.stack([bw_taps(1500.0 + 300.0 * c) for c in range(ch)])
    notches = np.stack([notch(c) for c in range(ch)])
    anr_on = np.array([0, 1, 0, 2, 0], np.int32)
    oi, oq = rows(ch, 128, seed=2)
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, taps[0], taps[0], mixer=msdr.MIXER_NCO, mode=AM, osc_i=oi[0], osc_q=oq[0], biquad_nodes=[[lowpass()], [notches[0]]])
    chain.set_node_coefficients_channels(1, 0, 0, notches)
    chain.set_anr(anr_on)
    chain.set_osc_channels(0, oi, oq)
    chain.set_taps_channels(0, taps)
    x = rng.integers(-20000, 20001, (ch, n)).astype(np.int16)
    audio, meters = metered(ctx, chain, x, B)
    si, sq = at(oi, 0, n), at(oq, 0, n)
    for c in range(ch):
        want, i, q = oracle_row(orc, x[c], si[c], sq[c], lambda b: (AM, taps[c], taps[c]), {}, want_iq=True)
        want = orc.anr_q15(orc.anr_new(), anr_on[c], want)
        nodes = [orc.biquad_teensy_new([lowpass()]), orc.biquad_teensy_new([notches[c]])]
        for k in range(ticks):
            blk = want[k * B:(k + 1) * B]
            for nd in nodes:
                blk = orc.biquad_teensy_update(nd, blk)
            want[k * B:(k + 1) * B] = blk
        assert np.array_equal(audio[c], want), c
        assert np.array_equal(meters[:, c], sums(i, q, n, B)), c
    chain.close()


def test_twelve_receivers_on_one_antenna_row(ctx, orc, golden):
    rng = np.random.default_rng(3603)
    ch, n = 12, 3 * B
    modes, ti, tq = mixed_bank(golden, ch)
    oi, oq = rows(ch, 128, seed=4)
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, ti[0], tq[0], mixer=msdr.MIXER_NCO, modes=modes, osc_i=oi[0], osc_q=oq[0])
    for _ in range(2):                                                   # (twice, as tools/pc_kernels_digest.py calls it)
        chain.set_input_rows(np.zeros(ch, np.int64), 1)
    chain.set_osc_channels(0, oi, oq)
    chain.set_taps_channels(0, ti, tq)
    x = rng.integers(-30000, 30001, (1, n)).astype(np.int16)
    audio, meters = metered(ctx, chain, x, B, ch=ch)
    si, sq = at(oi, 0, n), at(oq, 0, n)
    for c in range(ch):
        want, i, q = oracle_row(orc, x[0], si[c], sq[c], lambda b: (modes[c], ti[c], tq[c]), {}, want_iq=True)
        assert np.array_equal(audio[c], want), c
        assert np.array_equal(meters[:, c], sums(i, q, n, B)), c
    chain.close()


def call(ctx, chain, x):
    dy = ctx.array(x.shape, np.int16)
    chain.process(ctx.to_device(np.ascontiguousarray(x)), dy, x.shape[1])
    return dy.download()


def test_set_cleared_and_set_again_between_guard_words(ctx, orc):
    """d_meter carved from a larger array with sentinel entries before and behind; cleared: the next call leaves the buffer alone; a failing
    call writes nothing; the pointer survives reset, a retune of taps and a decimation switch"""
    rng = np.random.default_rng(3604)
    ch, n = 5, 3 * B
    taps = np.stack([bw_taps(1200.0 + 300.0 * c) for c in range(ch)])
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    chain = nco_chain(ctx, ch, taps, taps, steps, phases, mode=USB)
    assert chain.meter() is None
    x = rng.integers(-30000, 30001, (ch, n)).astype(np.int16)
    si, sq = Bank(steps, phases).advance(n)
    want = [oracle_row(orc, x[c], si[c], sq[c], lambda b: (USB, taps[c], taps[c]), {}, want_iq=True) for c in range(ch)]
    expect = np.stack([sums(want[c][1], want[c][2], n, B) for c in range(ch)], axis=1)          # [calls, ch]
    guard = 3
    first, second = (ctx.to_device(np.full(guard + ch + guard, SENTINEL, np.uint64)) for _ in range(2))

    def inside(buf):
        back = buf.download()
        assert (back[:guard] == SENTINEL).all() and (back[guard + ch:] == SENTINEL).all()
        return back[guard:guard + ch]

    chain.set_meter(first.offset(8 * guard))
    assert chain.meter() == first.ptr + 8 * guard
    assert np.array_equal(call(ctx, chain, x[:, :B]), np.stack([w[0][:B] for w in want]))
    assert np.array_equal(inside(first), expect[0])
    with pytest.raises(msdr.MsdrError) as e:                            # a misaligned pointer: nothing changed
        chain.set_meter(second.offset(8 * guard + 4))
    assert e.value.status == ARG and chain.meter() == first.ptr + 8 * guard
    chain.set_meter(None)
    assert chain.meter() is None
    first.upload(np.full(guard + ch + guard, SENTINEL, np.uint64))
    assert np.array_equal(call(ctx, chain, x[:, B:2 * B]), np.stack([w[0][B:2 * B] for w in want]))
    assert (first.download() == SENTINEL).all()                         # off: the buffer is the caller's again
    assert chain.info()["kernel"].startswith("chain_q15pcn_kernel")     # ... and the chain stays in the per-receiver family
    chain.set_meter(second.offset(8 * guard))
    chain.set_decimation(4)
    with pytest.raises(msdr.MsdrError) as e:                            # n % D != 0: nothing enqueued, nothing written
        chain.process(ctx.to_device(np.ascontiguousarray(x[:, :130])), ctx.array((ch, 33), np.int16), 130)
    assert e.value.status == LEN and (second.download() == SENTINEL).all()
    chain.set_decimation(1)
    assert chain.meter() == second.ptr + 8 * guard
    assert np.array_equal(call(ctx, chain, x[:, 2 * B:]), np.stack([w[0][2 * B:] for w in want]))
    assert np.array_equal(inside(second), expect[2]) and (first.download() == SENTINEL).all()
    chain.reset()
    chain.set_taps_channels(0, taps)
    chain.set_nco_channels(0, u32(steps), u32(phases))
    assert chain.meter() == second.ptr + 8 * guard
    call(ctx, chain, x[:, :B])
    assert np.array_equal(inside(second), expect[0])                    # from a clear history again
    chain.close()


def test_graphs_and_the_block_kernel_step_aside(ctx):
    rng = np.random.default_rng(3605)
    ch, T = 6, 2
    taps = np.stack([bw_taps(900.0 + 400.0 * c) for c in range(ch)])
    oi, oq = rows(1, 128, seed=8)
    a, control = (msdr.Chain(ctx, msdr.ARITH_Q15, ch, taps[0], taps[0], mixer=msdr.MIXER_NCO, mode=USB, osc_i=oi[0], osc_q=oq[0]) for _ in range(2))
    for o in (a, control):
        o.set_taps_channels(0, taps)
        o.set_block_kernel_q15(True)
    dxs, dys = [ctx.array((ch, B), np.int16) for _ in range(T)], [ctx.array((ch, B), np.int16) for _ in range(T)]
    g = a.graph(dxs, dys, B)                                             # made before the meter
    x = rng.integers(-20000, 20001, (ch, 2 * B)).astype(np.int16)
    assert np.array_equal(call(ctx, a, x[:, :B]), call(ctx, control, x[:, :B]))
    assert a.info()["kernel"].startswith("chain_q15pcb_kernel")
    buf = ctx.array((ch,), np.uint64).fill(0)
    a.set_meter(buf)
    for f in (g.launch, lambda: a.graph(dxs, dys, B)):
        with pytest.raises(msdr.MsdrError) as e:
            f()
        assert e.value.status == ARG
    a.set_block_kernel_q15(True)                                         # accepted; the call runs the unfused launches
    assert np.array_equal(call(ctx, a, x[:, B:]), call(ctx, control, x[:, B:]))
    assert a.info()["kernel"].startswith("chain_q15pc_kernel") and control.info()["kernel"].startswith("chain_q15pcb_kernel")
    assert buf.download().min() > 0
    a.set_meter(None)
    with pytest.raises(msdr.MsdrError) as e:                            # the graph of before knows nothing of what happened since
        g.launch()
    assert e.value.status == ARG
    g.close()
    g2 = a.graph(dxs, dys, B)                                            # without a meter the chain is capturable again
    g2.close()
    for o in (a, control):
        o.close()
