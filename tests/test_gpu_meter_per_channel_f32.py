"""The per-receiver S-meter (F32): msdr_chain_set_meter on fp32 chains -- one double per channel, the sum of both fp32 FIR outputs' squares over
the call (in_scale units), from the metered flavours of chain_f32pc / pco / pcn / pcnd.

Reference: for channel c, orclib.Oracle.chain_f32 with that channel's taps and oscillator in mode AM and no cascade, whatever the chain's own
mode: its output is sqrt(I^2 + Q^2), so S_orc = sum(audio.astype(float64) ** 2) over the call's outputs (within 1e-9 .. 7e-9 of the all-float64
value for 102 taps at n = 1000 .. 4600: the reference is far inside the tolerance).
Tolerance: |S_gpu - S_orc| <= 2.5e-5 S_orc.  It follows from the chain's own accuracy clause: e_go < 1e-5 on the AM audio gives
|sum g^2 - sum w^2| <= e (2 + e) sum w^2; the margin covers the square root's and the accumulation's roundings.  Every case prints its ratio
(about 1e-7 is expected).  The meter is also bit-identical between two runs of the same calls: no atomics, a fixed order."""
import numpy as np
import pytest

import orclib
from f32pc_cases import B, FS4, bw_taps, cascade
from gpuhelp import ctx, msdr, rel_rms  # noqa: F401
from test_gpu_decim_per_channel import step_list
from test_gpu_meter_per_channel import metered
from test_gpu_nco_per_channel import Bank, off_grid_steps, u32
from test_gpu_nco_per_channel_f32 import any_table, f32
from test_gpu_osc_per_channel_f32 import at, mixed_bank, rows, signal

pytestmark = pytest.mark.gpu
AM, LSB, USB, CW, SYNCAM = orclib.AM, orclib.LSB, orclib.USB, orclib.CW, orclib.SYNCAM
ARG = msdr.STATUS_ARGUMENT_ERROR
TOL = 2.5e-5
KINDS = ("shared table", "table per channel", "nco")
KERNEL = {"shared table": "chain_f32pc_kernel", "table per channel": "chain_f32pco_kernel", "nco": "chain_f32pcn_kernel"}


def bank_of(ctx, kind, rng, ch, n, modes, ti, tq, **kw):
    """(a maker of chains of one oscillator policy, the per-sample oscillator values si, sq [ch, n] of its model)"""
    if kind == "nco":
        steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
        si, sq = Bank(steps, phases).advance(n)

        def make():
            chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, ti[0], tq[0], mixer=msdr.MIXER_NCO, modes=modes, **any_table(), **kw)
            chain.set_taps_channels_f32(0, ti, tq)
            chain.set_nco_channels(0, u32(steps), u32(phases))
            return chain
        return make, f32(si), f32(sq)
    oi, oq = rows(ch, 128, seed=5)
    if kind == "shared table":
        oi, oq = np.tile(oi[:1], (ch, 1)), np.tile(oq[:1], (ch, 1))

    def make():
        chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, ti[0], tq[0], mixer=msdr.MIXER_NCO, modes=modes, osc_i=oi[0], osc_q=oq[0], **kw)
        chain.set_taps_channels_f32(0, ti, tq)
        if kind == "table per channel":
            chain.set_osc_channels(0, oi, oq)
        return chain
    return make, at(oi, 0, n), at(oq, 0, n)


def s_orc(env, n, step, D=1):
    """the reference's meter of every call of `step` input samples over the first n, from the full-rate AM audio sqrt(I^2 + Q^2)"""
    e = env.astype(np.float64) ** 2
    return np.array([e[lo + D - 1:min(lo + step, n):D].sum() for lo in range(0, n, step)])


def judged(tag, got, want):
    worst = float((np.abs(got - want) / want).max())
    print("meter %s |S_gpu - S_orc| / S_orc = %.3e" % (tag, worst))
    assert np.all(want > 0) and np.all(np.abs(got - want) <= TOL * want), (tag, worst)


# ------------------------------------------------------------------------------------------------ 4a. every sliding-window geometry
@pytest.mark.parametrize("kind", KINDS)
def test_every_sliding_window_geometry(ctx, orc, kind):
    rng = np.random.default_rng(4100 + KINDS.index(kind))
    ch, n = 10, 6 * B
    modes, ti, tq = mixed_bank(ch)
    make, si, sq = bank_of(ctx, kind, rng, ch, n, modes, ti, tq)
    x = signal(rng, ch, n)
    env = [orc.chain_f32(x[c], AM, ti[c], tq[c], si[c], sq[c], None) for c in range(ch)]
    own = [orc.chain_f32(x[c], int(modes[c]), ti[c], tq[c], si[c], sq[c], None) for c in range(ch)]
    for step, tile in ((B, 128), (2 * B, 256), (n, 512)):
        a, b = make(), make()
        assert not a.info()["flavour"] & msdr.FLAVOUR_METER
        audio, meters = metered(ctx, a, x, step, adtype=np.float32, mdtype=np.float64)
        _, again = metered(ctx, b, x, step, adtype=np.float32, mdtype=np.float64)
        assert np.array_equal(meters.view(np.uint64), again.view(np.uint64)), step          # two fresh chains, the same calls: the same bits
        info = a.info()
        assert info["kernel"].startswith(KERNEL[kind]) and info["tile"] == tile and info["flavour"] & msdr.FLAVOUR_METER, info
        for c in range(ch):
            judged("%s step %d ch %d" % (kind, step, c), meters[:, c], s_orc(env[c], n, step))
            assert rel_rms(audio[c], own[c]) < 1e-5, (step, c)
        a.set_meter(None)                                                # the flavour bit exactly while a meter is set
        a.process(ctx.to_device(np.ascontiguousarray(x[:, :B])), ctx.array((ch, B), np.float32), B)
        assert not a.info()["flavour"] & msdr.FLAVOUR_METER and a.info()["kernel"].startswith(KERNEL[kind])
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------ 4b. the tail, 4c. segments
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n, segs", [(1001, 0), (4600, 0), (4600, 3)])
def test_the_tail_and_the_segments(ctx, orc, kind, n, segs):
    """1001: tile 512, the second tile partly live, the last live lane holding 1 of its 8 outputs.  4600: 9 tiles, in the launcher's 2 segments
    of 5 or in the 3 of 3 that time_segments asks for; the partials go through the reducer, in segment order: the same bits run to run."""
    rng = np.random.default_rng(4200 + n + segs + KINDS.index(kind))
    ch = 3
    modes, ti, tq = mixed_bank(ch)
    make, si, sq = bank_of(ctx, kind, rng, ch, n, modes, ti, tq, time_segments=segs)
    x = signal(rng, ch, n)
    a, b = make(), make()
    audio, meters = metered(ctx, a, x, n, adtype=np.float32, mdtype=np.float64)
    _, again = metered(ctx, b, x, n, adtype=np.float32, mdtype=np.float64)
    assert np.array_equal(meters.view(np.uint64), again.view(np.uint64))
    info = a.info()
    assert info["tile"] == 512 and info["time_segments"] == (1 if n == 1001 else segs or 2), info
    for c in range(ch):
        env = orc.chain_f32(x[c], AM, ti[c], tq[c], si[c], sq[c], None)
        judged("%s n %d segs %d ch %d" % (kind, n, segs, c), meters[:, c], s_orc(env, n, n))
        assert rel_rms(audio[c], orc.chain_f32(x[c], int(modes[c]), ti[c], tq[c], si[c], sq[c], None)) < 1e-5, c
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ the Fs/4 one-stream flavour
def test_the_fs4_one_stream_flavour(ctx, orc):
    rng = np.random.default_rng(4300)
    ch, n = 4, 2 * 256
    taps = np.stack([bw_taps(900.0 + 700.0 * c) for c in range(ch)])
    chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, taps[0], taps[0], mode=AM)
    chain.set_taps_channels_f32(0, taps)
    x = signal(rng, ch, n)
    audio, meters = metered(ctx, chain, x, 256, adtype=np.float32, mdtype=np.float64)
    info = chain.info()
    assert info["kernel"].startswith("chain_f32pc_kernel") and info["flavour"] & msdr.FLAVOUR_METER, info
    si, sq = np.tile(FS4[0], n // 4), np.tile(FS4[1], n // 4)
    for c in range(ch):
        env = orc.chain_f32(x[c], AM, taps[c], taps[c], si, sq, None)
        judged("fs4 ch %d" % c, meters[:, c], s_orc(env, n, 256))
        assert rel_rms(audio[c], env) < 1e-5, c
    chain.close()


# ------------------------------------------------------------------------------------------------ 4e. decimation
@pytest.mark.parametrize("D", [3, 4, 8])
def test_decimation(ctx, orc, D):
    """11 channels, mixed modes, a low-pass cascade behind the kernel: 768 D inputs in calls of 32, 128, 256 outputs and one of 768, and one
    call of 1001 outputs for the tail; the reference's full-rate envelope at [D - 1::D]"""
    rng = np.random.default_rng(4500 + D)
    steps = step_list(rng)
    ch = steps.size
    modes, ti, tq = mixed_bank(ch)
    phases = rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    n_tail, n = 1001 * D, 768 * D
    x = signal(rng, ch, n_tail)
    si, sq = Bank(steps, phases).advance(n_tail)
    si, sq = f32(si), f32(sq)
    env = [orc.chain_f32(x[c], AM, ti[c], tq[c], si[c], sq[c], None) for c in range(ch)]
    for nout in (32, 128, 256, 768, 1001):
        chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, ti[0], tq[0], mixer=msdr.MIXER_NCO, modes=modes, biquad_coeffs=cascade("lp"), **any_table())
        chain.set_taps_channels_f32(0, ti, tq)
        chain.set_nco_channels(0, u32(steps), u32(phases))
        chain.set_decimation(D)
        m = n_tail if nout == 1001 else n
        _, meters = metered(ctx, chain, x[:, :m], nout * D, D, adtype=np.float32, mdtype=np.float64)
        info = chain.info()
        assert info["kernel"].startswith("chain_f32pcnd_kernel") and info["flavour"] & msdr.FLAVOUR_METER and info["flavour"] & msdr.FLAVOUR_DECIMATED, info
        for c in range(ch):
            judged("D %d nout %d ch %d" % (D, nout, c), meters[:, c], s_orc(env[c], m, nout * D, D))
        chain.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_chain_as_it_was(ctx):
    rng = np.random.default_rng(4600)
    ch = 4
    taps = np.stack([bw_taps(1200.0 + 300.0 * c) for c in range(ch)])
    x = signal(rng, ch, 2 * B)
    buf = ctx.array((ch,), np.float64).fill(0xA5)

    def run(chain):
        dy = ctx.array((ch, 2 * B), np.float32)
        chain.process(ctx.to_device(x), dy, 2 * B)
        return dy.download()

    def refused(f):
        with pytest.raises(msdr.MsdrError) as e:
            f()
        assert e.value.status == ARG, e.value

    def pair(**kw):
        return [msdr.Chain(ctx, msdr.ARITH_F32, ch, taps[0], taps[0], mixer=msdr.MIXER_NCO, mode=AM, **any_table(), **kw) for _ in range(2)]

    sentinel = buf.download().copy()
    # a chain created with MSDR_CHAIN_SYNCAM_PLL; a chain with an LMS channel on
    pll, pll_control = pair(flags=msdr.CHAIN_SYNCAM_PLL)
    lms, lms_control = pair()
    for o in (lms, lms_control):
        o.set_anr(np.array([0, 1, 0, 0], np.int32))
    for a, control in ((pll, pll_control), (lms, lms_control)):
        refused(lambda: a.set_meter(buf))
        assert a.meter() is None
        ga, gb = run(a), run(control)
        assert np.array_equal(ga.view(np.uint32), gb.view(np.uint32)) and a.info() == control.info()
        assert not a.info()["flavour"] & msdr.FLAVOUR_TAPS_PC and np.array_equal(buf.download(), sentinel)          # not even the change of kernel
    # set_anr with a channel on while a meter is set; all off is accepted
    m, m_control = pair()
    for o in (m, m_control):
        o.set_taps_channels_f32(0, taps)
    m.set_meter(buf)
    refused(lambda: m.set_anr(np.array([0, 0, 1, 0], np.int32)))
    refused(lambda: m.set_anr(None, 1))
    m.set_anr(None, 0)
    refused(lambda: m.set_meter(buf.offset(4)))                          # a misaligned pointer
    assert m.meter() == buf.ptr
    ga, gb = run(m), run(m_control)
    assert np.array_equal(ga.view(np.uint32), gb.view(np.uint32))
    assert m.info()["flavour"] == m_control.info()["flavour"] | msdr.FLAVOUR_METER
    assert not np.array_equal(buf.download(), sentinel)
    # the block switch is accepted and such calls run the unfused launches; graphs are refused
    m.set_block_kernel(True)
    m_control.set_block_kernel(True)
    dxs, dys = [ctx.array((ch, B), np.int16) for _ in range(2)], [ctx.array((ch, B), np.float32) for _ in range(2)]
    refused(lambda: m.graph(dxs, dys, B))
    dy = ctx.array((ch, B), np.float32)
    m.process(ctx.to_device(np.ascontiguousarray(x[:, :B])), dy, B)
    assert m.info()["kernel"].startswith("chain_f32pc_kernel") and not m.info()["flavour"] & msdr.FLAVOUR_BLOCK
    m_control.process(ctx.to_device(np.ascontiguousarray(x[:, :B])), dy, B)
    assert m_control.info()["flavour"] & msdr.FLAVOUR_BLOCK
    for o in (pll, pll_control, lms, lms_control, m, m_control):
        o.close()
