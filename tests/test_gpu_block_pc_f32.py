"""msdr_chain_set_block_kernel: a block-cadence call of an fp32 chain in per-channel mode as ONE launch (chain_f32pcb_kernel,
minimal-sdr_amd/csrc/msdr_chain_f32pcb.hiph) -- mixer, FIR, demodulator, CMSIS-order cascade, int16 conversion and the next FIR history.

The fused kernel executes the unfused launches' operations in the same order, so its outputs, the history and the cascade's pState are
theirs BIT FOR BIT: identity is derived, the tests assert it with np.array_equal against a twin chain that never gets the call.  The fused
chain alone is judged by f32judge (the project's contract: 1e-5 relative RMS against the oracle, the float64 clause at level 1).

Shapes: 5 channels (a partial group of 4 per wave) and 21 (a second workgroup, partial); blocks of 32, 128, 512 (4, 4 and 1 channel per
wave... the three geometries); 6 taps (np 8: head steps only) and 102 (np 104: 26 steps = 2 head steps + whole groups of 3); Fs/4 and a
128-entry oscillator table (shared, and per-channel rows); 0, 1, 2, 4 stages with shared and per-channel rows; fp32 and int16 out; AM / LSB /
USB mixed; 4 ticks."""
import ctypes as C
import itertools

import numpy as np
import pytest

import cascade_pc_cases as cc
import orclib
from f32judge import fp32_noise, judge, references
from f32pc_cases import FS4, bw_taps, hilbert_pair, nco128
from gpuhelp import ctx, msdr  # noqa: F401

pytestmark = pytest.mark.gpu
AM, LSB, USB = orclib.AM, orclib.LSB, orclib.USB
PCB, PCF = "chain_f32pcb_kernel", "chain_f32pc"
TICKS = 4


def bank(ch, nt):
    """modes AM / LSB / USB in turn; every channel taps of its own: AM rows of different bandwidths, the Hilbert pair scaled per channel"""
    modes = np.array([(AM, LSB, USB)[c % 3] for c in range(ch)], np.int32)
    ssb = hilbert_pair(nt)
    ci = np.stack([bw_taps(600.0 + 150.0 * c, nt) if modes[c] == AM else ssb[0] * np.float32(1 - 0.01 * c) for c in range(ch)])
    cq = np.stack([ci[c] if modes[c] == AM else ssb[1] * np.float32(1 - 0.01 * c) for c in range(ch)])
    return modes, ci, cq


def osc_rows(ch):
    k = np.arange(128)
    a = 2 * np.pi * (1 + 3 * np.arange(ch))[:, None] * k[None, :] / 128 + 0.3 * np.arange(ch)[:, None]
    q = lambda v: (np.round(32767 * v).astype(np.int16) / 32768.0).astype(np.float32)          # noqa: E731
    return q(np.sin(a)), q(np.cos(a))


def make(ctx, ch, nt, nco, rows, shared_rows, i16, block, osc_pc=False, flags=0):
    """a chain in per-channel mode: rows = [ch, S, 5] cascade rows or None; shared_rows: every channel runs rows[0] from one shared row"""
    modes, ci, cq = bank(ch, nt)
    osc = nco128(3) if nco else (None, None)
    chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, [ci[0], ci[1]], [cq[0], cq[1]], mixer=msdr.MIXER_NCO if nco else msdr.MIXER_FS4, modes=modes,
                       tapsets=(modes != AM).astype(np.int32), osc_i=osc[0], osc_q=osc[1], biquad_coeffs=None if rows is None else rows[0],
                       flags=flags | (msdr.CHAIN_OUT_I16 if i16 else 0))
    if block == "before":
        chain.set_block_kernel(1)
    chain.set_taps_channels_f32(0, ci, cq)
    if rows is not None and not shared_rows:
        chain.set_biquad_coeffs_channels(0, rows)
    if osc_pc:
        oi, oq = osc_rows(ch)
        chain.set_osc_channels(0, oi, oq)
    if block == "after":
        chain.set_block_kernel(1)
    return chain


def call(ctx, chain, x, i16):
    ch, n = x.shape
    dx, dy = ctx.to_device(np.ascontiguousarray(x)), ctx.array((ch, n), np.int16 if i16 else np.float32)
    chain.process(dx, dy, n)
    return dy.download()


def same_state(a, b, ch, tag):
    for c in sorted({0, ch // 2, ch - 1}):
        assert np.array_equal(a.fir_history(c), b.fir_history(c)), (tag, "history", c)
        if a.stages:
            assert np.array_equal(a.cmsis_state(c), b.cmsis_state(c)), (tag, "pState", c)


# (stages, shared rows): every stage count, both kinds of table
CASCADES = [(0, False), (1, True), (2, False), (4, False), (4, True), (1, False)]


# ------------------------------------------------------------------------------------------------ 1. bit identity
@pytest.mark.parametrize("nco", [False, True], ids=["fs4", "osc128"])
@pytest.mark.parametrize("nt", [6, 102])
@pytest.mark.parametrize("n", [32, 128, 512])
def test_fused_ticks_are_the_unfused_ticks_bit_for_bit(ctx, n, nt, nco):
    seen = set()
    for k, (stages, shared) in enumerate(CASCADES):
        ch = (5, 21)[k % 2]
        i16 = bool((k // 2 + (n // 32) + nt) % 2)
        osc_pc = nco and k % 3 == 0
        seen.add((ch, i16))
        rows = None if stages == 0 else cc.stage_rows(ch, stages, offset=k)
        if shared and rows is not None:
            rows = np.tile(rows[:1], (ch, 1, 1))
        a = make(ctx, ch, nt, nco, rows, shared, i16, ("before", "after")[k % 2], osc_pc)
        b = make(ctx, ch, nt, nco, rows, shared, i16, None, osc_pc)
        x = cc.signal(1000 * n + 10 * nt + k, ch, TICKS * n)
        tag = (n, nt, nco, stages, shared, ch, i16, osc_pc)
        if osc_pc:
            # set_osc_channels left a pending generation: calls are unfused until the history has turned over (test 3 holds the hand-over
            # itself); the TICKS judged below start behind it, on both chains alike
            warm = cc.signal(7000 + k, ch, n)
            for _ in range(-(-a.fir_history(0).size // n)):
                assert np.array_equal(call(ctx, a, warm, i16), call(ctx, b, warm, i16)), (tag, "warm-up")
        for t in range(TICKS):
            ga, gb = call(ctx, a, x[:, t * n:(t + 1) * n], i16), call(ctx, b, x[:, t * n:(t + 1) * n], i16)
            assert np.array_equal(ga, gb), (tag, t)
            assert a.info()["kernel"].startswith(PCB), (tag, t, a.info())
            assert np.abs(ga.astype(np.float64)).max() > (30 if i16 else 1e-3), (tag, t)
        ia, ib = a.info(), b.info()
        assert ia["kernel"].startswith(PCB) and ib["kernel"].startswith(PCF) and not ib["kernel"].startswith(PCB), (tag, ia, ib)
        want = msdr.FLAVOUR_BLOCK | msdr.FLAVOUR_TAPS_PC | (msdr.FLAVOUR_OSC_PC if osc_pc else 0) | (msdr.FLAVOUR_SEQ_CASCADE if stages else 0) | \
            (msdr.FLAVOUR_CASCADE_PC if stages and not shared else 0)
        assert ia["flavour"] == want, (tag, hex(ia["flavour"]), hex(want))
        assert ia["time_segments"] == 1 and ia["lds_bytes"] <= 64 * 1024, (tag, ia)
        same_state(a, b, ch, tag)
        a.close()
        b.close()
    assert seen == set(itertools.product((5, 21), (False, True))), seen


# ------------------------------------------------------------------------------------------------ 2. accuracy of the fused chain alone
@pytest.mark.parametrize("nco", [False, True], ids=["fs4", "osc128"])
def test_fused_chain_holds_the_fp32_contract(ctx, orc, nco):
    ch, n, nt = 5, 128, 102
    modes, ci, cq = bank(ch, nt)
    fam = cc.family()
    rows = np.stack([fam[c % 3] if modes[c] == AM else fam[3] for c in range(ch)])          # (SSB channels: the low-pass alone)
    chain = make(ctx, ch, nt, nco, rows, False, False, "after")
    x = cc.signal(77, ch, TICKS * n)
    got = np.concatenate([call(ctx, chain, x[:, t * n:(t + 1) * n], False) for t in range(TICKS)], axis=1)
    assert chain.info()["kernel"].startswith(PCB)
    osc = nco128(3) if nco else FS4
    for c in range(ch):
        case = cc.case_of(modes[c], ci[c], cq[c], rows[c], osc)
        e_go, e_gpu, e_orc, bound = judge(got[c], x[c], case, refs=references(x[c], case))
        b1 = 2 * e_orc + fp32_noise(case["bq"]) + 1e-6
        print("fused %s ch %d mode %d e_go %.3e e_gpu %.3e e_orc %.3e bound %.3e" % ("osc128" if nco else "fs4", c, modes[c], e_go, e_gpu, e_orc, b1))
        assert e_go < 1e-5, (c, "first clause", e_go)
        assert e_gpu <= min(bound, b1), (c, "float64 clause", e_gpu, b1)
    chain.close()


# ------------------------------------------------------------------------------------------------ 3. interleaving with unfused calls
def test_fused_and_unfused_calls_interleave_on_one_history_phase_and_state(ctx):
    ch, n, nt = 5, 128, 102
    rows = cc.stage_rows(ch, 2)
    a, b = make(ctx, ch, nt, True, rows, False, False, "after"), make(ctx, ch, nt, True, rows, False, False, None)
    oi, oq = osc_rows(ch)
    x = cc.signal(31, ch, 8 * n)
    pos = 0
    seen = []

    def both(m, tag):
        nonlocal pos
        ga, gb = call(ctx, a, x[:, pos:pos + m], False), call(ctx, b, x[:, pos:pos + m], False)
        pos += m
        assert np.array_equal(ga, gb), tag
        seen.append(a.info()["kernel"].startswith(PCB))
        assert not b.info()["kernel"].startswith(PCB), tag

    both(n, "fused tick")
    both(100, "a 100-sample call")
    both(n, "fused tick at another table position")
    for c in (a, b):
        c.set_osc_channels(1, oi[1:3], oq[1:3])          # a pending generation: unfused until the history has turned over
    both(n, "tick under a pending generation")
    both(n, "fused again")
    both(n, "and again")
    assert seen == [True, False, True, False, True, True], seen
    same_state(a, b, ch, "interleaved")
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 4. live row rewrites between fused ticks
def test_row_rewrites_between_fused_ticks_take_effect_over_the_old_history_and_state(ctx):
    ch, n, nt = 5, 128, 102
    rows, new_rows = cc.stage_rows(ch, 2), cc.stage_rows(ch, 2, offset=3)
    new_taps = bw_taps(3300.0, nt)
    a, b, keep = (make(ctx, ch, nt, False, rows, False, True, blk) for blk in ("after", None, "after"))
    x = cc.signal(41, ch, 4 * n)
    for t in range(4):
        if t == 2:
            for c in (a, b):
                c.set_taps_channels_f32(0, new_taps[None])                   # channel 0: AM
                c.set_biquad_coeffs_channels(3, new_rows[3:4])
        ga, gb, gk = (call(ctx, c, x[:, t * n:(t + 1) * n], True) for c in (a, b, keep))
        assert np.array_equal(ga, gb), t
        assert a.info()["kernel"].startswith(PCB), t
        for c in range(ch):
            assert np.array_equal(ga[c], gk[c]) == (t < 2 or c not in (0, 3)), (t, c)
    same_state(a, b, ch, "rewritten")
    for c in (a, b, keep):
        c.close()


# ------------------------------------------------------------------------------------------------ 5. graph replay
def test_graph_of_fused_ticks_replays_and_is_refused_after_what_it_cannot_know(ctx):
    ch, n, nt = 5, 128, 102
    rows = cc.stage_rows(ch, 2)
    a, b = make(ctx, ch, nt, True, rows, False, True, None), make(ctx, ch, nt, True, rows, False, True, None)
    xs = [ctx.array((ch, n), np.int16) for _ in range(TICKS)]
    ys = [ctx.array((ch, n), np.int16) for _ in range(TICKS)]
    with pytest.raises(msdr.MsdrError, match="not capturable") as e:          # the block kernel off: refused as ever
        a.graph(xs, ys, n)
    assert e.value.status == msdr.STATUS_ARGUMENT_ERROR
    a.set_block_kernel(1)
    g = a.graph(xs, ys, n)
    x = cc.signal(51, ch, 3 * TICKS * n)
    pos = 0

    def replay(tag):
        nonlocal pos
        for t in range(TICKS):
            xs[t].upload(x[:, pos + t * n:pos + (t + 1) * n])
        g.launch()
        for t in range(TICKS):
            want = call(ctx, b, x[:, pos + t * n:pos + (t + 1) * n], True)
            assert np.array_equal(ys[t].download(), want), (tag, t)
        pos += TICKS * n

    replay("first replay")
    replay("second replay")
    same_state(a, b, ch, "replayed")
    new_taps = bw_taps(3300.0, nt)
    for c in (a, b):
        c.set_taps_channels_f32(0, new_taps[None])                           # a row rewrite: the captured launches read the table
    replay("after a row rewrite")

    def refused(tag):
        with pytest.raises(msdr.MsdrError) as e:
            g.launch()
        assert e.value.status == msdr.STATUS_ARGUMENT_ERROR, tag

    oi, oq = osc_rows(ch)
    block = np.zeros((ch, n), np.int16)
    for tag, change in (("set_osc_channels", lambda c: c.set_osc_channels(1, oi[1:2], oq[1:2])),
                        ("set_mode", lambda c: c.set_mode(0, AM, 0)),
                        ("reset", lambda c: c.reset()),
                        ("set_block_kernel(0)", lambda c: c.set_block_kernel(0)),
                        ("one direct call", lambda c: call(ctx, c, block, True))):
        fresh = make(ctx, ch, nt, True, rows, False, True, "after")
        g2 = fresh.graph(xs, ys, n)
        g2.launch()
        change(fresh)
        with pytest.raises(msdr.MsdrError) as e:
            g2.launch()
        assert e.value.status == msdr.STATUS_ARGUMENT_ERROR, tag
        g2.close()
        fresh.close()
    g.close()
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals_and_the_chains_that_keep_the_unfused_path(ctx):
    f = ctx.lib.msdr_chain_set_block_kernel
    assert f(None, C.c_int(1)) == msdr.STATUS_ARGUMENT_ERROR
    q = msdr.Chain(ctx, msdr.ARITH_Q15, 4, np.zeros(102, np.int16), np.zeros(102, np.int16), mode=AM)
    assert f(q.h, C.c_int(1)) == msdr.STATUS_ARGUMENT_ERROR
    with pytest.raises(msdr.MsdrError) as e:
        q.set_block_kernel(1)
    assert e.value.status == msdr.STATUS_ARGUMENT_ERROR
    q.close()
    ch, n, nt = 5, 128, 102
    x = cc.signal(61, ch, n)
    lms = make(ctx, ch, nt, False, None, False, False, "after")
    lms.set_anr(np.array([0, 1, 0, 0, 0], np.int32))
    call(ctx, lms, x, False)
    assert lms.info()["kernel"].startswith(PCF) and not lms.info()["kernel"].startswith(PCB), lms.info()
    lms.set_anr(None, 0)                                                      # the LMS channel off again: fused from the next call on
    call(ctx, lms, x, False)
    call(ctx, lms, x, False)
    assert lms.info()["kernel"].startswith(PCB), lms.info()
    pll = make(ctx, ch, nt, False, None, False, False, "before", flags=msdr.CHAIN_SYNCAM_PLL)
    call(ctx, pll, x, False)
    assert pll.info()["kernel"].startswith(PCF) and not pll.info()["kernel"].startswith(PCB), pll.info()
    plain = msdr.Chain(ctx, msdr.ARITH_F32, ch, bw_taps(2400.0), bw_taps(2400.0), mode=AM)          # never in per-channel mode: the call changes nothing
    plain.set_block_kernel(1)
    call(ctx, plain, x, False)
    assert plain.info()["kernel"].startswith("chain_mfb_kernel"), plain.info()
    for c in (lms, pll, plain):
        c.close()
