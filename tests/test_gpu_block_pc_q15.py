"""msdr_chain_set_block_kernel_q15: a block-cadence call of a Q15 chain in per-channel mode as ONE launch (chain_q15pcb_kernel,
minimal-sdr_amd/csrc/msdr_chain_q15pcb.hiph) -- mixer, FIR pair, demodulator, the AudioFilterBiquad nodes from every channel's own records and
the next FIR history -- in place of chain_q15pc[o]_kernel + a node kernel + history[_rows]_kernel.

All arithmetic is integer and every sample goes through the unfused kernels' own functions, so identity is a requirement, not a tolerance:
every comparison is np.array_equal, against a twin chain that never gets the call and, for one case, against the oracle's Q15 chain.

Shapes: 5 channels (a partial wave of 4) and 9 (a partial workgroup of 16); blocks of 32, 128, 256, 512 (4, 4, 2 and 1 channel per wave); 8
taps (np 8: one step), 102 (np 104) and 250 (np 256: the history is longer than a 128 block); Fs/4, the shared 128-entry table and
per-channel rows; AM / LSB / USB mixed, both square roots; 0, 1, 2 nodes with uniform records (one of them of two stages) and per-channel
records of 1 .. 4 stages that differ between neighbours; one case of taps 32767 / -32768 under full-scale input (the accumulators wrap)."""
import ctypes as C

import numpy as np
import pytest

import orclib
from gpuhelp import ctx, msdr  # noqa: F401

pytestmark = pytest.mark.gpu
B = 128
L = 128
CORR = orclib.AUDIO_SAMPLE_RATE_EXACT / 24000.0
AM, LSB, USB, SYNCAM = orclib.AM, orclib.LSB, orclib.USB, orclib.SYNCAM
PCB, PC = "chain_q15pcb_kernel", "chain_q15pc"          # (PC: chain_q15pc_kernel and chain_q15pco_kernel)


def bw_taps(bw, n):
    return msdr.calc_fir_coeffs(n, float(bw), 70.0, 0, 0.0, 24000.0)[:n].copy()


def osc_rows(ch, seed=0):
    """(osc_i, osc_q) [ch, L]: a different bin and a different start phase per channel"""
    k = (1 + seed + 3 * np.arange(ch)) % L
    ph = 0.37 * (1 + seed) + 0.61 * np.arange(ch)
    a = 2 * np.pi * k[:, None] * np.arange(L)[None, :] / L + ph[:, None]
    return np.round(32767 * np.sin(a)).astype(np.int16), np.round(32767 * np.cos(a)).astype(np.int16)


def lowpass(c=0):
    return msdr.biquad_design(msdr.BQ_LOWPASS, np.float32((5400.0 - 90.0 * c) * CORR), 0.54)


def notch(c=0):
    return msdr.biquad_design(msdr.BQ_NOTCH, np.float32((3000.0 + 37.0 * c) * CORR), 15.0)


def stage_coef(nd, c, s):
    return (lowpass(3 * c + s) if (nd + s) % 2 == 0 else notch(5 * c + s))


def pc_stage_count(nd, c):
    return 1 + (c + 2 * nd) % 4          # 1 .. 4, neighbouring channels differ


def bank(ch, nt, seed, extreme=False):
    """modes AM / LSB / USB in turn; every channel taps of its own"""
    rng = np.random.default_rng(seed)
    modes = np.array([(AM, LSB, USB)[c % 3] for c in range(ch)], np.int32)
    if extreme:
        ti = np.where(rng.integers(0, 2, (ch, nt)) > 0, 32767, -32768).astype(np.int16)
        tq = np.where(rng.integers(0, 2, (ch, nt)) > 0, 32767, -32768).astype(np.int16)
    else:
        ti = np.stack([bw_taps(600.0 + 250.0 * c, nt) if modes[c] == AM else rng.integers(-2500, 2501, nt).astype(np.int16) for c in range(ch)])
        tq = np.stack([ti[c] if modes[c] == AM else rng.integers(-2500, 2501, nt).astype(np.int16) for c in range(ch)])
    return modes, ti, tq


def make(ctx, ch, nt, mixer, nodes, on, sqrt_kind=msdr.SQRT_F32, seed=0, extreme=False, flags=0, modes=None):
    """a Q15 chain in per-channel mode.  mixer: "fs4", "shared" (the NCO table of the configuration) or "rows" (per-channel rows, which leave a
    pending generation); nodes: (count, "uni" | "uni2" | "pc"); on: None, or "before" / "after" -- where set_block_kernel_q15(1) is called"""
    m, ti, tq = bank(ch, nt, seed, extreme)
    if modes is not None:
        m = np.asarray(modes, np.int32)
    count, kind = nodes
    uniform = [[lowpass()], [notch()]] if kind != "uni2" else [[lowpass(), notch(3)], [notch()]]
    oi, oq = osc_rows(ch, seed)
    kw = dict(mixer=msdr.MIXER_NCO, osc_i=oi[0], osc_q=oq[0]) if mixer != "fs4" else {}
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, ti[0], tq[0], modes=m, sqrt_kind=sqrt_kind, biquad_nodes=uniform[:count], flags=flags, **kw)
    if on == "before":
        chain.set_block_kernel_q15(1)
    chain.set_taps_channels(0, ti, tq)
    if mixer == "rows":
        chain.set_osc_channels(0, oi, oq)
    if kind == "pc":
        for nd in range(count):
            for c in range(ch):
                for s in range(pc_stage_count(nd, c)):
                    chain.set_node_coefficients_channels(nd, c, s, stage_coef(nd, c, s)[None])
    if on == "after":
        chain.set_block_kernel_q15(1)
    return chain


def call(ctx, chain, x):
    ch, n = x.shape
    dx, dy = ctx.to_device(np.ascontiguousarray(x)), ctx.array((ch, n), np.int16)
    chain.process(dx, dy, n)
    return dy.download()


def turn_over(ctx, chains, ch, n, seed):
    """calls until the history holds no sample of an earlier oscillator generation (set_osc_channels): unfused on every chain, and equal"""
    x = np.random.default_rng(seed).integers(-20000, 20001, (ch, n)).astype(np.int16)
    for _ in range(-(-chains[0].fir_history(0).size // n)):
        outs = [call(ctx, c, x) for c in chains]
        for o in outs[1:]:
            assert np.array_equal(outs[0], o), "warm-up"


def same_history(a, b, ch, tag):
    for c in range(ch):
        assert np.array_equal(a.fir_history(c), b.fir_history(c)), (tag, "history", c)


def fused(chain):
    return chain.info()["kernel"].startswith(PCB)


def unfused(chain):
    k = chain.info()["kernel"]
    return k.startswith(PC) and not k.startswith(PCB)


# ------------------------------------------------------------------------------------------------ 1. identity with the unfused launches
#         id                      ch  n    nt   mixer     sqrt             nodes        extreme
CASES = [("fs4-5-128-102-2uni",   5, 128, 102, "fs4",    msdr.SQRT_F32, (2, "uni"),  False),
         ("rows-9-128-102-2pc",   9, 128, 102, "rows",   msdr.SQRT_Q31, (2, "pc"),   False),
         ("shared-5-32-250-1pc",  5, 32,  250, "shared", msdr.SQRT_F32, (1, "pc"),   False),
         ("rows-9-256-8-0",       9, 256, 8,   "rows",   msdr.SQRT_Q31, (0, "uni"),  False),
         ("fs4-9-512-102-1uni",   9, 512, 102, "fs4",    msdr.SQRT_Q31, (1, "uni"),  False),
         ("shared-9-128-250-uni2", 9, 128, 250, "shared", msdr.SQRT_Q31, (2, "uni2"), False),
         ("rows-5-512-250-2pc",   5, 512, 250, "rows",   msdr.SQRT_F32, (2, "pc"),   False),
         ("fs4-5-256-8-2pc",      5, 256, 8,   "fs4",    msdr.SQRT_F32, (2, "pc"),   False),
         ("shared-5-32-8-2uni",   5, 32,  8,   "shared", msdr.SQRT_Q31, (2, "uni"),  False),
         ("rows-5-128-102-wrap",  5, 128, 102, "rows",   msdr.SQRT_F32, (2, "uni"),  True)]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_fused_ticks_are_the_unfused_ticks_bit_for_bit(ctx, case):
    tag, ch, n, nt, mixer, sqrt_kind, nodes, extreme = case
    k = [c[0] for c in CASES].index(tag)
    a = make(ctx, ch, nt, mixer, nodes, ("before", "after")[k % 2], sqrt_kind, seed=k, extreme=extreme)
    b = make(ctx, ch, nt, mixer, nodes, None, sqrt_kind, seed=k, extreme=extreme)
    rng = np.random.default_rng(1000 + k)
    if mixer == "rows":
        turn_over(ctx, [a, b], ch, n, 2000 + k)
    ticks = 10
    x = rng.choice(np.array([-32768, 32767], np.int16), (ch, ticks * n)) if extreme else rng.integers(-30000, 30001, (ch, ticks * n)).astype(np.int16)

    def both(t, want_a, want_b, what):
        ga, gb = call(ctx, a, x[:, t * n:(t + 1) * n]), call(ctx, b, x[:, t * n:(t + 1) * n])
        assert np.array_equal(ga, gb), (tag, what, t)
        assert fused(a) == want_a and unfused(a) == (not want_a), (tag, what, t, a.info())
        assert fused(b) == want_b and unfused(b) == (not want_b), (tag, what, t, b.info())
        for chain, want in ((a, want_a), (b, want_b)):           # which kernel ran the nodes: the block kernel's third phase, or a kernel behind
            if want:
                assert chain.node_kernel() == ("chain_q15pcb_kernel" if nodes[0] else ""), (tag, what, t, chain.node_kernel())
            elif nodes[1] == "pc":
                assert chain.node_kernel() == "biquad_teensy_pc_kernel<%d>" % nodes[0], (tag, what, t, chain.node_kernel())
            else:
                assert chain.node_kernel() != "chain_q15pcb_kernel" and (chain.node_kernel() == "") == (nodes[0] == 0), (tag, what, t, chain.node_kernel())
        return ga

    loud = 0
    for t in range(6):
        loud = max(loud, int(np.abs(both(t, True, False, "fused | unfused").astype(np.int32)).max()))
    assert loud > 30, (tag, loud)                                   # (the comparison is not one of silences)
    ia = a.info()
    want_tile = {32: 128, 128: 128, 256: 256, 512: 512}[n]
    assert ia["tile"] == want_tile and ia["taps_padded"] == (nt + 7) // 8 * 8 and ia["time_segments"] == 1 and ia["flavour"] == 0, (tag, ia)
    assert 0 < ia["lds_bytes"] <= 64 * 1024 and ia["block"] in (64, 128, 256) and ia["grid"] >= 1, (tag, ia)
    assert ia["grid"] * (ia["block"] // 64) * (512 // want_tile) >= ch, (tag, ia)
    same_history(a, b, ch, tag)
    # the node records by continuation: the fused twin carries on unfused ...
    a.set_block_kernel_q15(0)
    for t in range(6, 8):
        both(t, False, False, "unfused behind fused")
    # ... and the other way round
    b.set_block_kernel_q15(1)
    for t in range(8, 10):
        both(t, False, True, "fused behind unfused")
    same_history(a, b, ch, tag + " end")
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 2. the oracle
def test_fused_bank_is_the_oracle_per_receiver(ctx, orc):
    """per-channel taps, oscillator rows and notches; 5 channels x 128, one tick under the pending generation and 4 fused ticks"""
    ch, nt, ticks = 5, 102, 5
    modes = np.array([AM, LSB, USB, AM, AM], np.int32)
    rng = np.random.default_rng(7)
    ti = np.stack([bw_taps(700.0 + 500.0 * c, nt) if modes[c] == AM else rng.integers(-2500, 2501, nt).astype(np.int16) for c in range(ch)])
    tq = np.stack([ti[c] if modes[c] == AM else rng.integers(-2500, 2501, nt).astype(np.int16) for c in range(ch)])
    oi, oq = osc_rows(ch, 4)
    lp = lowpass()
    nrows = np.stack([notch(7 * c) for c in range(ch)])
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, ti[0], tq[0], mixer=msdr.MIXER_NCO, modes=modes, osc_i=oi[0], osc_q=oq[0], biquad_nodes=[[lp], [notch()]])
    chain.set_taps_channels(0, ti, tq)
    chain.set_osc_channels(0, oi, oq)
    chain.set_node_coefficients_channels(1, 0, 0, nrows)
    chain.set_block_kernel_q15(1)
    x = rng.integers(-30000, 30001, (ch, ticks * B)).astype(np.int16)
    got = np.empty_like(x)
    for t in range(ticks):
        got[:, t * B:(t + 1) * B] = call(ctx, chain, x[:, t * B:(t + 1) * B])
        assert fused(chain) == (t > 0), (t, chain.info())          # (tick 0: the history still holds samples of the table before set_osc_channels)
        assert chain.node_kernel() == ("chain_q15pcb_kernel" if t > 0 else "biquad_teensy_pc_kernel<2>"), (t, chain.node_kernel())
    for c in range(ch):
        st = {}
        nodes = [orc.biquad_teensy_new([lp]), orc.biquad_teensy_new([nrows[c]])]
        for t in range(ticks):
            sl = slice(t * B, (t + 1) * B)
            w = orc.chain_q15(x[c, sl], int(modes[c]), ti[c], tq[c], mixer=1, osc_i=oi[c], osc_q=oq[c], state=st)
            for nd in nodes:
                w = orc.biquad_teensy_update(nd, w)
            assert np.array_equal(got[c, sl], w), (c, t)
    chain.close()


# ------------------------------------------------------------------------------------------------ 3. shared IF
@pytest.mark.parametrize("ni", [1, 2])
def test_shared_if_rows_and_a_live_change_of_the_map(ctx, ni):
    ch, n, nt = 5, 128, 102
    maps = [np.array([0, 0, 0, 0, 0] if ni == 1 else [1, 0, 0, 1, 1], np.uint32), np.array([0, 0, 0, 0, 0] if ni == 1 else [0, 1, 0, 1, 0], np.uint32)]
    a = make(ctx, ch, nt, "shared", (2, "pc"), "after", seed=3)
    b = make(ctx, ch, nt, "shared", (2, "pc"), None, seed=3)          # the twin: the identity, fed replicated rows
    rng = np.random.default_rng(30 + ni)

    def tick(rows, tag):
        xin = rng.integers(-30000, 30001, (ch if rows is None else ni, n)).astype(np.int16)
        full = np.full((ch, n), 0x5A5A, np.int16)                    # (the shared rows at the start of a buffer of the replicated size)
        full.reshape(-1)[:xin.size] = xin.reshape(-1)
        dx, dy = ctx.to_device(full), ctx.array((ch, n), np.int16)
        a.process(dx, dy, n)
        assert np.array_equal(dy.download(), call(ctx, b, xin if rows is None else xin[rows])), tag
        assert fused(a) and unfused(b), (tag, a.info(), b.info())
        same_history(a, b, ch, tag)                                  # every receiver keeps its own history: what IT heard

    a.set_input_rows(maps[0], ni)
    for t in range(2):
        tick(maps[0], ("first map", t))
    a.set_input_rows(maps[1], ni)                                    # an antenna switch between ticks
    for t in range(2):
        tick(maps[1], ("second map", t))
    a.set_input_rows(None)                                           # back to the identity
    for t in range(2):
        tick(None, ("identity", t))
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 4. fallbacks
def test_calls_the_fused_kernel_does_not_take_run_unfused_and_equal(ctx):
    ch, n, nt = 5, 128, 102
    rng = np.random.default_rng(40)
    x = rng.integers(-30000, 30001, (ch, 8 * n)).astype(np.int16)

    def pair(a, b, xs, want, tag):
        ga, gb = call(ctx, a, xs), call(ctx, b, xs)
        assert np.array_equal(ga, gb), tag
        assert fused(a) == want and unfused(a) == (not want) and unfused(b), (tag, a.info(), b.info())

    # another block length
    a, b = make(ctx, ch, nt, "shared", (2, "pc"), "after"), make(ctx, ch, nt, "shared", (2, "pc"), None)
    pair(a, b, x[:, :n], True, "a tick")
    pair(a, b, x[:, n:n + 130], False, "130 samples")
    pair(a, b, x[:, n + 130:2 * n + 130], True, "a tick at another table position")
    # a pending oscillator generation: one history length (103 samples: one tick), fused again afterwards
    oi, oq = osc_rows(ch, 9)
    for c in (a, b):
        c.set_osc_channels(1, oi[1:3], oq[1:3])
    pair(a, b, x[:, 3 * n:4 * n], False, "under a pending generation")
    pair(a, b, x[:, 4 * n:5 * n], True, "fused again")
    pair(a, b, x[:, 5 * n:6 * n], True, "and again")
    # an LMS channel on, and off again
    for c in (a, b):
        c.set_anr(np.array([0, 1, 0, 2, 0], np.int32))
    pair(a, b, x[:, 6 * n:7 * n], False, "an LMS channel on")
    for c in (a, b):
        c.set_anr(None, 0)
    pair(a, b, x[:, 7 * n:8 * n], True, "LMS off")
    same_history(a, b, ch, "fallbacks")
    a.close()
    b.close()
    # a SYNCAM channel under the PLL
    modes = [AM, SYNCAM, LSB, AM, SYNCAM]
    a = make(ctx, ch, nt, "shared", (2, "uni"), "before", flags=msdr.CHAIN_SYNCAM_PLL, modes=modes)
    b = make(ctx, ch, nt, "shared", (2, "uni"), None, flags=msdr.CHAIN_SYNCAM_PLL, modes=modes)
    for t in range(2):
        pair(a, b, x[:, t * n:(t + 1) * n], False, ("PLL", t))
    a.close()
    b.close()
    # never in per-channel mode: the switch changes nothing
    am = bw_taps(2400.0, nt)
    plain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, am, am, mode=AM)
    plain.set_block_kernel_q15(1)
    call(ctx, plain, x[:, :n])
    assert plain.info()["kernel"].startswith("chain_q15mb_kernel"), plain.info()
    plain.close()


# ------------------------------------------------------------------------------------------------ 5. graph replay
def test_graph_of_fused_ticks_replays_and_is_refused_after_what_it_cannot_know(ctx):
    ch, n, nt, ticks = 5, 128, 102, 4
    a, b = make(ctx, ch, nt, "rows", (2, "pc"), "after", seed=5), make(ctx, ch, nt, "rows", (2, "pc"), None, seed=5)
    turn_over(ctx, [a, b], ch, n, 50)
    xs = [ctx.array((ch, n), np.int16) for _ in range(ticks)]
    ys = [ctx.array((ch, n), np.int16) for _ in range(ticks)]
    g = a.graph(xs, ys, n)
    x = np.random.default_rng(51).integers(-30000, 30001, (ch, 4 * ticks * n)).astype(np.int16)
    pos = 0

    def replay(tag):
        nonlocal pos
        for t in range(ticks):
            xs[t].upload(x[:, pos + t * n:pos + (t + 1) * n])
        g.launch()
        for t in range(ticks):
            want = call(ctx, b, x[:, pos + t * n:pos + (t + 1) * n])
            assert np.array_equal(ys[t].download(), want), (tag, t)
        pos += ticks * n
        same_history(a, b, ch, tag)

    replay("first replay")
    replay("second replay")
    new_taps = bw_taps(3300.0, nt)
    for c in (a, b):
        c.set_taps_channels(0, new_taps[None])                                # a row rewrite: the captured launches read the table
    replay("after a row rewrite")
    assert pc_stage_count(1, 2) == 1
    for c in (a, b):
        c.set_node_coefficients_channels(1, 2, 1, notch(40)[None])            # channel 2, node 1: one stage -> two (the flag is in the record)
    replay("after a change of stage count")
    assert unfused(b)
    call(ctx, a, x[:, :n])                                                     # (what the chain itself runs now)
    assert fused(a)
    g.close()
    a.close()
    b.close()

    oi, oq = osc_rows(ch, 11)
    block = np.zeros((ch, n), np.int16)
    for tag, change in (("set_osc_channels", lambda c: c.set_osc_channels(1, oi[1:2], oq[1:2])),
                        ("set_mode", lambda c: c.set_mode(0, AM, 0)),
                        ("reset", lambda c: c.reset()),
                        ("set_block_kernel_q15(0)", lambda c: c.set_block_kernel_q15(0)),
                        ("set_anr", lambda c: c.set_anr(None, 0)),
                        ("one direct call", lambda c: call(ctx, c, block))):
        fresh = make(ctx, ch, nt, "shared", (2, "pc"), "after", seed=5)
        g2 = fresh.graph(xs, ys, n)
        g2.launch()
        change(fresh)
        with pytest.raises(msdr.MsdrError) as e:
            g2.launch()
        assert e.value.status == msdr.STATUS_ARGUMENT_ERROR, tag
        g2.close()
        fresh.close()


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals(ctx):
    f = ctx.lib.msdr_chain_set_block_kernel_q15
    assert f(None, C.c_int(1)) == msdr.STATUS_ARGUMENT_ERROR
    taps = np.zeros(102, np.float32)
    taps[50] = 1.0
    f32 = msdr.Chain(ctx, msdr.ARITH_F32, 4, taps, taps, mode=AM)
    assert f(f32.h, C.c_int(1)) == msdr.STATUS_ARGUMENT_ERROR
    with pytest.raises(msdr.MsdrError) as e:
        f32.set_block_kernel_q15(1)
    assert e.value.status == msdr.STATUS_ARGUMENT_ERROR
    f32.close()
    q = msdr.Chain(ctx, msdr.ARITH_Q15, 4, np.zeros(102, np.int16), np.zeros(102, np.int16), mode=AM)
    assert ctx.lib.msdr_chain_set_block_kernel(q.h, C.c_int(1)) == msdr.STATUS_ARGUMENT_ERROR          # the fp32 switch keeps refusing Q15 chains
    q.set_block_kernel_q15(1)
    q.set_block_kernel_q15(0)
    q.close()
