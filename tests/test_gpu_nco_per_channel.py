"""Per-receiver phase-accumulator oscillator (Q15): msdr_chain_set_nco_channels tunes each receiver of the bank to ANY frequency -- tune() of
receiver rx (Minimal-SDR.ino:328-368) -- and chain_q15pcn_kernel computes channel ch's oscillator from its own {phase, step}.

The model here keeps one phase per channel and sample, phi += the step in force, and turns the phases into oscillator values with
msdr.nco_q15 (the host definition, held to a numpy restatement of its formulas by tests/test_nco_host.py).  Those per-sample values feed
orclib.Oracle.chain_q15 one channel and one 128-sample block at a time -- the reference's "owner rewrites Osc_I_buffer_i / Osc_Q_buffer_i
before each update()" (freq_conv.h:33-34) -- so the oracle's FIR state holds samples mixed with the oscillator of their own time.
Everything is int16 and bit-exact: np.array_equal, no tolerance."""
import ctypes as C

import numpy as np
import pytest

import orclib
from gpuhelp import ctx, msdr  # noqa: F401
from test_gpu_osc_per_channel import bw_taps, lowpass, mixed_bank, notch, oracle_row, pad, rows, run

pytestmark = pytest.mark.gpu
B = 128
NT = 102
PCN = "chain_q15pcn_kernel"
AM, LSB, USB, CW, SYNCAM = orclib.AM, orclib.LSB, orclib.USB, orclib.CW, orclib.SYNCAM
M32 = np.uint64(0xFFFFFFFF)


class Bank:
    """the model: phase of the NEXT sample and step per channel"""

    def __init__(self, steps, phases=None):
        self.step = np.asarray(steps, np.uint64).copy()
        self.phi = np.zeros(self.step.size, np.uint64) if phases is None else np.asarray(phases, np.uint64).copy()

    def retune(self, first, steps, phases=None):
        steps = np.asarray(steps, np.uint64)
        self.step[first:first + steps.size] = steps
        if phases is not None:
            self.phi[first:first + steps.size] = np.asarray(phases, np.uint64)

    def advance(self, n):
        """(osc_i "sin", osc_q "cos") [ch, n] of the next n samples; the phases move on"""
        ph = (self.phi[:, None] + np.arange(n, dtype=np.uint64)[None, :] * self.step[:, None]) & M32
        s, c = msdr.nco_q15(ph.astype(np.uint32))
        self.phi = (self.phi + np.uint64(n) * self.step) & M32
        return s.reshape(ph.shape), c.reshape(ph.shape)

    def reset(self):
        self.phi[:] = 0

    def check(self, chain, tag=""):
        for c in range(self.step.size):
            assert chain.nco(c) == (int(self.step[c]), int(self.phi[c])), (tag, c)


def u32(a):
    return np.asarray(a, np.uint64).astype(np.uint32)


def any_table():
    """the tables a chain with the table mixer is created with; nothing reads them once the oscillator is a phase accumulator"""
    oi, oq = rows(1, 128, seed=3)
    return dict(osc_i=oi[0], osc_q=oq[0])


def off_grid_steps(rng, n):
    return rng.integers(1, 1 << 32, n, dtype=np.uint64) | np.uint64(1)


# ------------------------------------------------------------------------------------------------ 1. ticks and one long call
def test_ticks_and_one_long_call(ctx, orc, golden):
    """11 channels (two groups of 4 and a partial one; one channel per step of the list: 0, 5 * 2^25, fs / 4, -fs / 4, one LSB below zero and six
    seeded ones), 102 taps, AM / LSB / USB / CW; 6 ticks of 128 (4 channels per wave), 3 calls of 256 (2 per wave) and ONE call of 768 (1 per
    wave)"""
    rng = np.random.default_rng(1001)
    n = 6 * B
    steps = np.concatenate([np.array([0, 5 << 25, 0x40000000, 0xC0000000, 0xFFFFFFFF], np.uint64), rng.integers(0, 1 << 32, 6, dtype=np.uint64)])
    ch = steps.size
    assert ch == 11 and ch % 4 and len(set(steps.tolist())) == ch
    modes, ti, tq = mixed_bank(golden, ch)
    phases = rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    x = rng.integers(-30000, 30001, (ch, n)).astype(np.int16)
    outs = []
    for step, tile in ((B, 128), (2 * B, 256), (n, 512)):
        chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, ti[0], tq[0], mixer=msdr.MIXER_NCO, modes=modes, **any_table())
        chain.set_taps_channels(0, ti, tq)
        chain.set_nco_channels(0, u32(steps), u32(phases))
        bank = Bank(steps, phases)
        bank.check(chain, "before the first call")
        got = np.empty_like(x)
        si, sq = np.empty_like(x), np.empty_like(x)
        for o in range(0, n, step):
            got[:, o:o + step] = run(ctx, chain, x[:, o:o + step])
            si[:, o:o + step], sq[:, o:o + step] = bank.advance(step)
            bank.check(chain, (step, o))
        outs.append(got)
        info = chain.info()
        assert info["kernel"].startswith(PCN) and info["tile"] == tile, info
        if step == B:          # pcn_lds_bytes: 4 waves x 4 channels of chain_q15pc_kernel's area (no row per channel) + ONE 4 096-byte sine table
            assert info["lds_bytes"] == 16 * 2 * (4 * (128 + 104) + 2 * 104) + 4096, info
        chain.close()
    for c in range(ch):
        want = oracle_row(orc, x[c], si[c], sq[c], lambda b: (modes[c], ti[c], tq[c]), {})
        assert np.array_equal(outs[0][c], want), c
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


# ------------------------------------------------------------------------------------------------ 2. bit-identity with the table path
def test_on_the_128_grid_the_chain_equals_the_table_chain(ctx, golden):
    """steps k_c * 2^25, start phases j_c * 2^25: the twin chain gets set_osc_channels rows built from msdr.nco_q15 at osc_len 128"""
    rng = np.random.default_rng(1002)
    ch, n = 9, 4 * B
    modes, ti, tq = mixed_bank(golden, ch)
    k = np.array([0, 1, 5, 32, 64, 96, 127, 77, 3], np.uint64)
    j = np.array([0, 0, 17, 1, 127, 64, 5, 90, 33], np.uint64)
    ph = (((j[:, None] + k[:, None] * np.arange(128, dtype=np.uint64)[None, :]) << np.uint64(25)) & M32).astype(np.uint32)
    s, c = msdr.nco_q15(ph)
    oi, oq = s.reshape(ch, 128), c.reshape(ch, 128)
    x = rng.integers(-30000, 30001, (ch, n)).astype(np.int16)
    a = msdr.Chain(ctx, msdr.ARITH_Q15, ch, ti[0], tq[0], mixer=msdr.MIXER_NCO, modes=modes, osc_i=oi[0], osc_q=oq[0])
    b = msdr.Chain(ctx, msdr.ARITH_Q15, ch, ti[0], tq[0], mixer=msdr.MIXER_NCO, modes=modes, osc_i=oi[0], osc_q=oq[0])
    for o in (a, b):
        o.set_taps_channels(0, ti, tq)
    a.set_nco_channels(0, u32(k << np.uint64(25)), u32(j << np.uint64(25)))
    b.set_osc_channels(0, oi, oq)
    for lo, hi in ((0, B), (B, 3 * B), (3 * B, 4 * B)):                  # a tick, a call of 256, a tick: the table position is 0 at each
        ga, gb = run(ctx, a, x[:, lo:hi]), run(ctx, b, x[:, lo:hi])
        assert np.array_equal(ga, gb), (lo, hi)
        assert np.abs(ga.astype(np.int32)).max() > 1000
    assert a.info()["kernel"].startswith(PCN) and b.info()["kernel"].startswith("chain_q15pco_kernel")
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 3. live retunes inside one history length
def test_live_retunes_inside_one_history_length(ctx, orc):
    """6 channels, 500 taps (arm_fir_init_q15 takes even counts only: 499 is refused at creation; a history of four calls), calls of 128: five
    retunes of different channel ranges behind calls 1 .. 4 -- two of them behind call 3 with no call in between (the bank between them never mixes a sample: not a generation), the one behind call 2 with
    explicit phases, the others phase-continuous"""
    rng = np.random.default_rng(1003)
    ch, nt, calls = 6, 500, 12
    taps = np.stack([bw_taps(600.0 + 300.0 * c, nt) for c in range(ch)])
    modes = np.array([(AM, LSB, USB, AM)[c % 4] for c in range(ch)], np.int32)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, taps[0], taps[0], mixer=msdr.MIXER_NCO, modes=modes, **any_table())
    chain.set_nco_channels(0, u32(steps), u32(phases))                  # (no per-channel taps yet: the table is filled from the shared set ...)
    chain.set_taps_channels(0, taps)                                    # (... and the two calls combine in this order too)
    bank = Bank(steps, phases)
    x = rng.integers(-30000, 30001, (ch, calls * B)).astype(np.int16)
    got, si, sq = np.empty_like(x), np.empty_like(x), np.empty_like(x)
    plan = {1: [(0, 2, False)], 2: [(1, 4, True)], 3: [(3, 3, False), (2, 3, False)], 4: [(0, 6, False)]}       # call -> (first, count, explicit phases)
    for k in range(calls):
        sl = slice(k * B, (k + 1) * B)
        got[:, sl] = run(ctx, chain, x[:, sl])
        assert chain.info()["kernel"].startswith(PCN)
        si[:, sl], sq[:, sl] = bank.advance(B)
        bank.check(chain, k)
        for first, count, explicit in plan.get(k, []):
            ns = off_grid_steps(rng, count)
            nph = rng.integers(0, 1 << 32, count, dtype=np.uint64) if explicit else None
            chain.set_nco_channels(first, u32(ns), None if nph is None else u32(nph))
            bank.retune(first, ns, nph)
            bank.check(chain, ("retuned", k))
    for c in range(ch):
        want = oracle_row(orc, x[c], si[c], sq[c], lambda b: (modes[c], taps[c], taps[c]), {})
        for k in range(calls):
            sl = slice(k * B, (k + 1) * B)
            assert np.array_equal(got[c, sl], want[sl]), (c, k)
    chain.close()


def test_seventeen_generations_inside_one_history_drop_the_oldest_only(ctx, orc):
    """1024 taps, ticks of 32: 20 retunes inside one history length; 16 generations are kept, so the samples of the four oldest are mixed with a
    later oscillator -- and the channels that never changed are exact all the same (one generation = the whole bank)"""
    rng = np.random.default_rng(1021)
    ch, nt, T = 5, 1024, 32
    ticks = 24
    taps = np.stack([bw_taps(900.0 + 500.0 * c, nt) for c in range(ch)])
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, taps[0], taps[0], mixer=msdr.MIXER_NCO, mode=LSB, **any_table())
    chain.set_taps_channels(0, taps)
    chain.set_nco_channels(0, u32(steps), u32(phases))
    bank = Bank(steps, phases)
    x = rng.integers(-30000, 30001, (ch, ticks * T)).astype(np.int16)
    got = np.empty_like(x)
    for k in range(ticks):
        got[:, k * T:(k + 1) * T] = run(ctx, chain, x[:, k * T:(k + 1) * T])
        if k < 20:
            chain.set_nco_channels(2, u32(off_grid_steps(rng, 1)))          # channel 2 only
    si, sq = bank.advance(ticks * T)
    for c in (0, 1, 3, 4):
        assert np.array_equal(got[c], oracle_row(orc, x[c], si[c], sq[c], lambda b: (LSB, taps[c], taps[c]), {})), c
    chain.close()


# ------------------------------------------------------------------------------------------------ 4. shared IF
@pytest.mark.parametrize("order", ["rows first", "nco first"])
def test_twelve_receivers_on_one_antenna_row(ctx, orc, order):
    rng = np.random.default_rng(1004)
    ch, n = 12, 3 * B
    taps = np.stack([bw_taps((600.0, 2400.0, 4000.0)[c % 3]) for c in range(ch)])
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    assert len(set(steps.tolist())) == ch
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, taps[0], taps[0], mixer=msdr.MIXER_NCO, mode=AM, **any_table())
    if order == "rows first":
        chain.set_input_rows(np.zeros(ch, np.int64), 1)
    chain.set_nco_channels(0, u32(steps), u32(phases))
    if order == "nco first":
        chain.set_input_rows(np.zeros(ch, np.int64), 1)
    chain.set_taps_channels(0, taps)
    x = rng.integers(-30000, 30001, (1, n)).astype(np.int16)
    got = np.empty((ch, n), np.int16)
    for o in range(0, n, B):
        dx, dy = ctx.to_device(np.ascontiguousarray(x[:, o:o + B])), ctx.array((ch, B), np.int16)
        chain.process(dx, dy, B)
        got[:, o:o + B] = dy.download()
    assert chain.info()["kernel"].startswith(PCN)
    si, sq = Bank(steps, phases).advance(n)
    for c in range(ch):
        assert np.array_equal(got[c], oracle_row(orc, x[0], si[c], sq[c], lambda b: (AM, taps[c], taps[c]), {})), c
    chain.close()


# ------------------------------------------------------------------------------------------------ 5. interplay and state
def test_interplay_with_nodes_pll_lms_and_the_other_setters(ctx, orc, golden):
    """two one-stage biquad nodes per channel, a SYNCAM channel under MSDR_CHAIN_SYNCAM_PLL and an LMS channel; set_taps_channels and set_mode
    between ticks; init_fir keeps the phases; reset zeroes phases and time and keeps the steps"""
    rng = np.random.default_rng(1005)
    ch, n = 6, 2 * B
    am = bw_taps(2400.0)
    sets_i = [am, pad(golden["taps/FIR_SSB_I_coeffs"])]
    sets_q = [am, pad(golden["taps/FIR_SSB_Q_coeffs"])]
    modes = np.array([AM, SYNCAM, LSB, AM, USB, AM], np.int32)
    tapsets = np.array([0, 0, 1, 0, 1, 0], np.int32)
    anr_on = np.array([0, 0, 0, 1, 0, 0], np.int32)
    lp = lowpass()
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, sets_i, sets_q, mixer=msdr.MIXER_NCO, modes=modes, tapsets=tapsets, biquad_nodes=[[lp], [notch(0)]],
                       flags=msdr.CHAIN_SYNCAM_PLL, **any_table())
    chain.set_anr(anr_on)
    # every receiver near the 6 kHz carrier of its test signal
    steps = np.array([msdr.nco_step(6000.0 + 13.7 * c - 20.0) for c in range(ch)], np.uint64)
    phases = rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    chain.set_nco_channels(0, u32(steps), u32(phases))
    bank = Bank(steps, phases)
    own = {}
    states = [{} for _ in range(ch)]
    nodes = [[orc.biquad_teensy_new([lp]), orc.biquad_teensy_new([notch(0)])] for _ in range(ch)]
    pll = [orc.syncam_new() for _ in range(ch)]
    anr = [orc.anr_new() for _ in range(ch)]
    t0 = 0

    def coeffs(c):
        return (own[c], own[c]) if c in own else (sets_i[tapsets[c]], sets_q[tapsets[c]])

    def tick(tag, step):
        nonlocal t0
        t = t0 + np.arange(n)
        t0 += n
        x = np.stack([(9000 * (1 + 0.5 * np.sin(2 * np.pi * 400 * t / 24000)) * np.cos(2 * np.pi * 6000 * t / 24000 + c)
                       + 1500 * np.cos(2 * np.pi * 7000 * t / 24000) + rng.integers(-100, 101, n)).astype(np.int16) for c in range(ch)])
        got = run(ctx, chain, x, step)
        assert chain.info()["kernel"].startswith(PCN), tag
        si, sq = bank.advance(n)
        bank.check(chain, tag)
        for c in range(ch):
            pll_ch = modes[c] == SYNCAM
            audio, i_f, q_f = oracle_row(orc, x[c], si[c], sq[c], lambda b: ((AM if pll_ch else modes[c]),) + coeffs(c), states[c], want_iq=True)
            if pll_ch:
                audio = orc.syncam_q15(pll[c], i_f, q_f)
            audio = orc.anr_q15(anr[c], anr_on[c], audio)
            for nd in nodes[c]:
                audio = orc.biquad_teensy_update(nd, audio)
            assert np.array_equal(got[c], audio), (tag, c)

    tick("first", B)
    own[3] = bw_taps(1300.0)
    chain.set_taps_channels(3, own[3][None, :])
    tick("taps of its own", None)
    chain.set_mode(0, USB, 1)
    modes[0], tapsets[0] = USB, 1
    ns = np.array([msdr.nco_step(-5990.0), msdr.nco_step(6011.0)], np.uint64)
    chain.set_nco_channels(4, u32(ns))                                   # phase-continuous, a pending generation under the setters below
    bank.retune(4, ns)
    am2 = bw_taps(1800.0)
    chain.set_taps(0, am2, am2)                                          # a rebuild of the chain's tables: the bank and its generation go over
    sets_i[0] = sets_q[0] = am2
    tick("set_mode, retune, set_taps", B)
    chain.init_fir()                                                     # FIR state only: phases and steps carry on
    states = [{} for _ in range(ch)]
    bank.check(chain, "after init_fir")
    tick("init_fir", B)
    chain.reset()                                                        # time and phases to 0, the steps stay; PLL and LMS state cleared, the nodes' kept
    states = [{} for _ in range(ch)]
    pll = [orc.syncam_new() for _ in range(ch)]
    anr = [orc.anr_new() for _ in range(ch)]
    bank.reset()
    bank.check(chain, "after reset")
    tick("reset", 64)
    chain.close()


# ------------------------------------------------------------------------------------------------ 7. refusals leave the chain untouched
def test_refusals_leave_the_chain_untouched(ctx, orc):
    rng = np.random.default_rng(1007)
    ch = 6
    am = bw_taps(2400.0)
    oi, oq = rows(ch, 128)
    x = rng.integers(-20000, 20001, (ch, 2 * B)).astype(np.int16)
    steps, phases = u32(off_grid_steps(rng, ch)), u32(rng.integers(0, 1 << 32, ch, dtype=np.uint64))
    lib = ctx.lib
    ERR = msdr.STATUS_ARGUMENT_ERROR

    def call(chain, first, count, a, b=None):
        return lib.msdr_chain_set_nco_channels(None if chain is None else chain.h, C.c_uint32(first), C.c_uint32(count),
                                               None if a is None else a.ctypes.data_as(C.c_void_p), None if b is None else b.ctypes.data_as(C.c_void_p))

    def table_chain():
        return msdr.Chain(ctx, msdr.ARITH_Q15, ch, am, am, mixer=msdr.MIXER_NCO, mode=LSB, osc_i=oi[0], osc_q=oq[0])

    def same(a, b, tag):
        ga, gb = run(ctx, a, x, B), run(ctx, b, x, B)
        assert np.array_equal(ga, gb), tag
        assert a.info() == b.info(), tag
        return ga

    assert call(None, 0, ch, steps) == ERR
    fs4, fs4_control = (msdr.Chain(ctx, msdr.ARITH_Q15, ch, am, am, mode=AM) for _ in range(2))
    assert call(fs4, 0, ch, steps) == ERR                                             # the Fs/4 mixer has no oscillator to tune
    same(fs4, fs4_control, "fs4")
    a, a_control = table_chain(), table_chain()
    assert call(a, 0, ch, None, phases) == ERR                                        # a NULL step array
    assert call(a, 4, 3, steps) == ERR                                                # 4 .. 6 of 6
    assert call(a, ch, 1, steps) == ERR
    assert call(a, 1, ch - 1, steps) == ERR                                           # a partial first call
    assert call(a, 0, ch - 1, steps) == ERR
    assert call(a, 0, 0, None) == 0                                                   # count == 0 does nothing ...
    with pytest.raises(msdr.MsdrError):
        a.nco(0)                                                                      # ... the chain is not in the mode
    ga = same(a, a_control, "table chain")
    assert PCN not in a.info()["kernel"]
    for c in range(ch):
        assert np.array_equal(ga[c], orc.chain_q15(x[c], LSB, am, am, mixer=1, osc_i=oi[0], osc_q=oq[0])), c
    assert call(a, 0, ch, steps, phases) == ERR                                       # samples have been processed: the history is not clear
    same(a, a_control, "first call over a used history")
    a.init_fir()
    a_control.init_fir()
    assert call(a, 0, ch, steps, phases) == 0                                         # directly after init_fir it is
    run(ctx, a, x, B)
    assert a.info()["kernel"].startswith(PCN)
    a_control.close()
    b, b_control = table_chain(), table_chain()                                       # per-channel oscillator tables exclude the phase accumulator
    for o in (b, b_control):
        o.set_osc_channels(0, oi, oq)
    assert call(b, 0, ch, steps, phases) == ERR
    same(b, b_control, "table rows")
    # a chain in the mode refuses the table setters and graphs; its next output equals that of a twin that never saw those calls
    n1, n1_control = table_chain(), table_chain()
    for o in (n1, n1_control):
        o.set_nco_channels(0, steps, phases)
    with pytest.raises(msdr.MsdrError) as e:
        n1.set_osc(oi[0], oq[0])
    assert e.value.status == ERR
    with pytest.raises(msdr.MsdrError) as e:
        n1.set_osc_channels(0, oi, oq)
    assert e.value.status == ERR
    dxs, dys = [ctx.array((ch, B), np.int16) for _ in range(2)], [ctx.array((ch, B), np.int16) for _ in range(2)]
    with pytest.raises(msdr.MsdrError) as e:
        n1.graph(dxs, dys, B)
    assert e.value.status == ERR
    assert call(n1, 2, 5, steps) == ERR                                               # a range past `channels` on a chain in the mode
    g1 = same(n1, n1_control, "nco chain")
    assert n1.info()["kernel"].startswith(PCN)
    si, sq = Bank(steps, phases).advance(2 * B)
    for c in range(ch):
        assert np.array_equal(g1[c], oracle_row(orc, x[c], si[c], sq[c], lambda blk: (LSB, am, am), {})), c
    # a graph made before the first call is refused at launch afterwards
    g_chain = table_chain()
    g_chain.set_taps_channels(0, np.tile(am, (ch, 1)))                                # (chain_q15pc_kernel: a Q15 chain with a 128-entry table can be captured)
    g = g_chain.graph(dxs, dys, B)
    g_chain.set_nco_channels(0, steps, phases)
    with pytest.raises(msdr.MsdrError) as e:
        g.launch()
    assert e.value.status == ERR
    g.close()
    # the block-kernel switch is accepted and such calls run the unfused launches
    n1.set_block_kernel_q15(True)
    n1_control.set_block_kernel_q15(False)
    same(n1, n1_control, "block switch")
    assert n1.info()["kernel"].startswith(PCN)
    for o in (fs4, fs4_control, a, b, b_control, n1, n1_control, g_chain):
        o.close()
