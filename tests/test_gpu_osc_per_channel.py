"""Per-receiver oscillator tables (Q15): tune() of receiver rx moves that receiver's local oscillator and nothing else
(Minimal-SDR.ino:328-368), and AudioEffectFreqConv mixes with whatever Osc_I_buffer_i / Osc_Q_buffer_i hold at each update()
(freq_conv.cpp:70-103).  msdr_chain_set_osc_channels gives single channels table rows of their own; chain_q15pco_kernel mixes channel ch
with row ch.

The oracle (orclib.Oracle.chain_q15 takes the tables per call and keeps its state outside the configuration) is evaluated one channel and
one 128-sample block at a time with the table VALUES that were in force when each sample arrived: its FIR state holds mixed samples, which
is the rule "a history sample keeps the table of its own time".  Everything is int16 and bit-exact: np.array_equal, no tolerance."""
import ctypes as C

import numpy as np
import pytest

import orclib
from gpuhelp import ctx, msdr  # noqa: F401

pytestmark = pytest.mark.gpu
B = 128
NT = 102
CORR = orclib.AUDIO_SAMPLE_RATE_EXACT / 24000.0
PCO = "chain_q15pco_kernel"
AM, LSB, USB, CW, SYNCAM = orclib.AM, orclib.LSB, orclib.USB, orclib.CW, orclib.SYNCAM


def bw_taps(bw, n=NT):
    return msdr.calc_fir_coeffs(n, float(bw), 70.0, 0, 0.0, 24000.0)[:n].copy()


def pad(t, n=NT):
    return np.concatenate([np.zeros(n - t.size, np.int16), np.asarray(t, np.int16)])


def rows(ch, L, seed=0):
    """(osc_i, osc_q) [ch, L]: a different bin and a different start phase per channel"""
    k = (1 + seed + 3 * np.arange(ch)) % L
    ph = 0.37 * (1 + seed) + 0.61 * np.arange(ch)
    a = 2 * np.pi * k[:, None] * np.arange(L)[None, :] / L + ph[:, None]
    return np.round(32767 * np.sin(a)).astype(np.int16), np.round(32767 * np.cos(a)).astype(np.int16)


def at(tab, pos, n):
    """the values of every channel's row ([ch, L]) met by n samples from table position pos"""
    return tab[:, (pos + np.arange(n)) % tab.shape[1]]


def run(ctx, chain, x, step=None):
    ch, n = x.shape
    got = np.empty_like(x)
    step = step or n
    for o in range(0, n, step):
        m = min(step, n - o)
        dx, dy = ctx.to_device(np.ascontiguousarray(x[:, o:o + m])), ctx.array((ch, m), np.int16)
        chain.process(dx, dy, m)
        got[:, o:o + m] = dy.download()
    return got


def oracle_row(orc, x, oi, oq, cfg, state, want_iq=False):
    """one channel: x, oi, oq per SAMPLE (a multiple of 128 of them); cfg(block) -> (mode, coeffs_i, coeffs_q) of that block"""
    out = []
    for b in range(x.size // B):
        sl = slice(b * B, (b + 1) * B)
        mode, ci, cq = cfg(b)
        out.append(orc.chain_q15(x[sl], int(mode), ci, cq, mixer=1, osc_i=oi[sl], osc_q=oq[sl], state=state, want_iq=want_iq))
    return [np.concatenate(p) for p in zip(*out)] if want_iq else np.concatenate(out)


def mixed_bank(golden, ch):
    modes = np.array([(AM, LSB, USB, CW)[c % 4] for c in range(ch)], np.int32)
    ti = np.stack([bw_taps(500.0 + 350.0 * c) if modes[c] == AM else pad(golden["taps/FIR_CW_I_coeffs" if modes[c] == CW else "taps/FIR_SSB_I_coeffs"]) for c in range(ch)])
    tq = np.stack([ti[c] if modes[c] == AM else pad(golden["taps/FIR_CW_Q_coeffs" if modes[c] == CW else "taps/FIR_SSB_Q_coeffs"]) for c in range(ch)])
    return modes, ti, tq


def lowpass():
    return msdr.biquad_design(msdr.BQ_LOWPASS, np.float32(5400.0 * CORR), 0.54)


def notch(c):
    return msdr.biquad_design(msdr.BQ_NOTCH, np.float32((3000.0 + 0.37 * c) * CORR), 15.0)


# ------------------------------------------------------------------------------------------------ 1. ticks and one long call
@pytest.mark.parametrize("L", [128, 24])
def test_ticks_and_one_long_call(ctx, orc, golden, L):
    """10 channels (a partial group of 4), 102 taps, AM / LSB / USB / CW; 6 ticks of 128 (4 channels per wave), 3 calls of 256 (2 per wave) and ONE
    call of 768 (1 per wave); 128 % 24 != 0: the table position moves from tick to tick"""
    rng = np.random.default_rng(100 + L)
    ch, n = 10, 6 * B
    modes, ti, tq = mixed_bank(golden, ch)
    oi, oq = rows(ch, L)
    assert len({r.tobytes() for r in oi}) == ch
    x = rng.integers(-30000, 30001, (ch, n)).astype(np.int16)
    outs = []
    for step, tile in ((B, 128), (2 * B, 256), (n, 512)):
        chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, ti[0], tq[0], mixer=msdr.MIXER_NCO, modes=modes, osc_i=oi[0], osc_q=oq[0])
        chain.set_taps_channels(0, ti, tq)
        chain.set_osc_channels(0, oi, oq)
        outs.append(run(ctx, chain, x, step))
        info = chain.info()
        assert info["kernel"].startswith(PCO) and info["tile"] == tile, info
        chain.close()
    si, sq = at(oi, 0, n), at(oq, 0, n)
    for c in range(ch):
        want = oracle_row(orc, x[c], si[c], sq[c], lambda b: (modes[c], ti[c], tq[c]), {})
        assert np.array_equal(outs[0][c], want), c
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], outs[2])


# ------------------------------------------------------------------------------------------------ 2. live changes inside one history length
def test_live_changes_inside_one_history_length(ctx, orc, golden):
    """256 taps, ticks of 32: set_osc_channels on channels 3 .. 6 after ticks 2, 4 and 5 -- three generations inside one history --, the one
    after tick 4 as two calls in a row (the first one's rows never mix a sample); then set_osc for all rows"""
    rng = np.random.default_rng(2)
    ch, nt, T, L = 10, 256, 32, 128
    ticks = 24
    taps = np.stack([bw_taps(600.0 + 300.0 * c, nt) for c in range(ch)])
    modes = np.array([(AM, LSB, USB, AM)[c % 4] for c in range(ch)], np.int32)
    cur_i, cur_q = rows(ch, L)
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, taps[0], taps[0], mixer=msdr.MIXER_NCO, modes=modes, osc_i=cur_i[0], osc_q=cur_q[0])
    chain.set_taps_channels(0, taps)
    chain.set_osc_channels(0, cur_i, cur_q)
    x = rng.integers(-30000, 30001, (ch, ticks * T)).astype(np.int16)
    got = np.empty_like(x)
    si, sq = np.empty_like(x), np.empty_like(x)
    for k in range(ticks):
        sl = slice(k * T, (k + 1) * T)
        got[:, sl] = run(ctx, chain, x[:, sl])
        assert chain.info()["kernel"].startswith(PCO)
        si[:, sl], sq[:, sl] = at(cur_i, k * T, T), at(cur_q, k * T, T)
        if k in (2, 4, 5):
            ni, nq = rows(4, L, seed=10 + k)
            if k == 4:
                junk = rows(4, L, seed=77)
                chain.set_osc_channels(3, *junk)
            chain.set_osc_channels(3, ni, nq)
            cur_i, cur_q = cur_i.copy(), cur_q.copy()
            cur_i[3:7], cur_q[3:7] = ni, nq
        if k == 8:
            one = rows(1, L, seed=5)
            chain.set_osc(one[0][0], one[1][0])
            cur_i, cur_q = np.tile(one[0], (ch, 1)), np.tile(one[1], (ch, 1))
    for c in range(ch):
        want = oracle_row(orc, x[c], si[c], sq[c], lambda b: (modes[c], taps[c], taps[c]), {})
        for k in range(ticks):
            sl = slice(k * T, (k + 1) * T)
            assert np.array_equal(got[c, sl], want[sl]), (c, k)
    chain.close()


def test_seventeen_generations_inside_one_history_drop_the_oldest_only(ctx, orc):
    """1024 taps, ticks of 32: 20 changes inside one history length; 16 generations are kept, so the samples of the four oldest tables are
    mixed with a later table -- and the channels that never changed their row are exact all the same (one generation = the whole bank)"""
    rng = np.random.default_rng(21)
    ch, nt, T, L = 5, 1024, 32, 128
    ticks = 24
    taps = np.stack([bw_taps(900.0 + 500.0 * c, nt) for c in range(ch)])
    cur_i, cur_q = rows(ch, L)
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, taps[0], taps[0], mixer=msdr.MIXER_NCO, mode=LSB, osc_i=cur_i[0], osc_q=cur_q[0])
    chain.set_taps_channels(0, taps)
    chain.set_osc_channels(0, cur_i, cur_q)
    x = rng.integers(-30000, 30001, (ch, ticks * T)).astype(np.int16)
    got = np.empty_like(x)
    for k in range(ticks):
        got[:, k * T:(k + 1) * T] = run(ctx, chain, x[:, k * T:(k + 1) * T])
        if k < 20:
            chain.set_osc_channels(2, *rows(1, L, seed=30 + k))          # channel 2 only
    si, sq = at(cur_i, 0, ticks * T), at(cur_q, 0, ticks * T)
    for c in (0, 1, 3, 4):
        assert np.array_equal(got[c], oracle_row(orc, x[c], si[c], sq[c], lambda b: (LSB, taps[c], taps[c]), {})), c
    chain.close()


# ------------------------------------------------------------------------------------------------ 3. interplay
def test_interplay_with_the_other_setters(ctx, orc, golden):
    """set_taps_channels before and after, set_mode on a channel with its own row, set_taps on a shared set, init_fir, reset (rows kept,
    generations cleared), per-channel node coefficients with two biquad nodes: the oracle follows"""
    rng = np.random.default_rng(3)
    ch, L, n = 10, 24, 2 * B
    am = bw_taps(2400.0)
    sets_i = [am, pad(golden["taps/FIR_SSB_I_coeffs"])]
    sets_q = [am, pad(golden["taps/FIR_SSB_Q_coeffs"])]
    modes = np.array([(AM, LSB, USB, AM, AM)[c % 5] for c in range(ch)], np.int32)
    tapsets = np.array([(0, 1, 1, 0, 0)[c % 5] for c in range(ch)], np.int32)
    lp = lowpass()
    nrows = np.stack([notch(7 * c) for c in range(ch)])
    oi0, oq0 = rows(1, L, seed=9)
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, sets_i, sets_q, mixer=msdr.MIXER_NCO, modes=modes, tapsets=tapsets, osc_i=oi0[0], osc_q=oq0[0],
                       biquad_nodes=[[lp], [notch(0)]])
    cur_i, cur_q = np.tile(oi0, (ch, 1)), np.tile(oq0, (ch, 1))
    own = {}
    states = [{} for _ in range(ch)]
    nodes = [[orc.biquad_teensy_new([lp]), orc.biquad_teensy_new([notch(0)])] for _ in range(ch)]
    pos = 0

    def coeffs(c):
        return (own[c], own[c]) if c in own else (sets_i[tapsets[c]], sets_q[tapsets[c]])

    def tick(tag, step):
        nonlocal pos
        x = rng.integers(-25000, 25001, (ch, n)).astype(np.int16)
        got = run(ctx, chain, x, step)
        assert chain.info()["kernel"].startswith(PCO), tag
        si, sq = at(cur_i, pos, n), at(cur_q, pos, n)
        pos += n
        for c in range(ch):
            audio = oracle_row(orc, x[c], si[c], sq[c], lambda b: (modes[c],) + coeffs(c), states[c])
            for nd in nodes[c]:
                audio = orc.biquad_teensy_update(nd, audio)
            assert np.array_equal(got[c], audio), (tag, c)

    def retable(first, count, seed):
        nonlocal cur_i, cur_q
        ni, nq = rows(count, L, seed=seed)
        chain.set_osc_channels(first, ni, nq)
        cur_i, cur_q = cur_i.copy(), cur_q.copy()
        cur_i[first:first + count], cur_q[first:first + count] = ni, nq

    own[0] = bw_taps(900.0)                                            # set_taps_channels BEFORE the first per-channel oscillator call
    chain.set_taps_channels(0, own[0][None, :])
    retable(0, ch, 1)
    tick("first", B)
    own[3] = bw_taps(1300.0)                                           # ... and after
    chain.set_taps_channels(3, own[3][None, :])
    tick("taps after", None)
    chain.set_mode(0, USB, 1)                                          # back on a shared set, another mode: the row of channel 0 stays
    modes[0], tapsets[0] = USB, 1
    del own[0]
    retable(4, 3, 2)
    tick("set_mode", 64)
    am2 = bw_taps(1800.0)
    chain.set_taps(0, am2, am2)                                        # a rebuild of the chain's tables: the bank and its pending generation go over
    sets_i[0] = sets_q[0] = am2
    tick("set_taps", B)
    chain.set_node_coefficients_channels(1, 0, 0, nrows)
    for c in range(ch):
        orc.lib.orc_biquad_teensy_set_coefficients(C.byref(nodes[c][1]), C.c_uint32(0), orclib._ptr(np.ascontiguousarray(nrows[c], np.int32)))
    retable(8, 2, 3)
    tick("node rows", B)
    chain.init_fir()                                                   # FIR state only; the table position carries on
    states = [{} for _ in range(ch)]
    tick("init_fir", B)
    retable(1, 2, 4)
    chain.reset()                                                      # the rows are kept, the pending generation is gone with the history
    states = [{} for _ in range(ch)]
    pos = 0
    tick("reset", 32)
    chain.close()


def test_a_syncam_channel_under_the_pll_and_an_lms_channel(ctx, orc):
    rng = np.random.default_rng(31)
    ch, L, n = 6, 128, 6 * B
    t = np.arange(n)
    x = np.stack([(9000 * (1 + 0.5 * np.sin(2 * np.pi * 400 * t / 24000)) * np.cos(2 * np.pi * 6000 * t / 24000 + c)
                   + 1500 * np.cos(2 * np.pi * 7000 * t / 24000) + rng.integers(-100, 101, n)).astype(np.int16) for c in range(ch)])
    taps = np.stack([bw_taps(2000.0 + 400.0 * c) for c in range(ch)])
    modes = np.array([AM, SYNCAM, AM, AM, SYNCAM, AM], np.int32)
    anr_on = np.array([0, 0, 1, 2, 0, 0], np.int32)
    # every receiver near its own carrier: bins 30 .. 35 of 128 (6000 Hz is bin 32)
    a = 2 * np.pi * (30 + np.arange(ch))[:, None] * np.arange(L)[None, :] / L + 0.3 * np.arange(ch)[:, None]
    oi, oq = np.round(32767 * np.sin(a)).astype(np.int16), np.round(32767 * np.cos(a)).astype(np.int16)
    for step in (B, 2 * B):
        chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, taps[0], taps[0], mixer=msdr.MIXER_NCO, modes=modes, osc_i=oi[0], osc_q=oq[0], flags=msdr.CHAIN_SYNCAM_PLL)
        chain.set_anr(anr_on)
        chain.set_osc_channels(0, oi, oq)
        chain.set_taps_channels(0, taps)
        got = run(ctx, chain, x, step)
        assert chain.info()["kernel"].startswith(PCO)
        si, sq = at(oi, 0, n), at(oq, 0, n)
        for c in range(ch):
            audio, i_f, q_f = oracle_row(orc, x[c], si[c], sq[c], lambda b: (AM, taps[c], taps[c]), {}, want_iq=True)
            if modes[c] == SYNCAM:
                audio = orc.syncam_q15(orc.syncam_new(), i_f, q_f)
            audio = orc.anr_q15(orc.anr_new(), anr_on[c], audio)
            assert np.array_equal(got[c], audio), (step, c)
        chain.close()


# ------------------------------------------------------------------------------------------------ 4. refusals leave the chain untouched
def test_refusals_leave_the_chain_untouched(ctx, orc):
    rng = np.random.default_rng(4)
    ch, L = 6, 128
    am = bw_taps(2400.0)
    oi, oq = rows(ch, L)
    x = rng.integers(-20000, 20001, (ch, 2 * B)).astype(np.int16)
    lib = ctx.lib

    def call(chain, first, count, a, b):
        return lib.msdr_chain_set_osc_channels(chain.h, C.c_uint32(first), C.c_uint32(count), None if a is None else a.ctypes.data_as(C.c_void_p),
                                               None if b is None else b.ctypes.data_as(C.c_void_p))

    fs4, fs4_control = (msdr.Chain(ctx, msdr.ARITH_Q15, ch, am, am, mode=AM) for _ in range(2))
    assert call(fs4, 0, ch, oi, oq) == msdr.STATUS_ARGUMENT_ERROR                     # the Fs/4 mixer has no tables
    assert lib.msdr_chain_set_osc_channels(None, C.c_uint32(0), C.c_uint32(1), oi.ctypes.data_as(C.c_void_p), oq.ctypes.data_as(C.c_void_p)) == msdr.STATUS_ARGUMENT_ERROR
    nco, nco_control = (msdr.Chain(ctx, msdr.ARITH_Q15, ch, am, am, mixer=msdr.MIXER_NCO, mode=LSB, osc_i=oi[0], osc_q=oq[0]) for _ in range(2))
    assert call(nco, 0, ch, None, oq) == msdr.STATUS_ARGUMENT_ERROR                   # a NULL array, either one
    assert call(nco, 0, ch, oi, None) == msdr.STATUS_ARGUMENT_ERROR
    assert call(nco, 4, 3, oi, oq) == msdr.STATUS_ARGUMENT_ERROR                      # 4 .. 6 of 6
    assert call(nco, ch, 1, oi, oq) == msdr.STATUS_ARGUMENT_ERROR
    assert call(nco, 0, 0, None, None) == 0                                           # count == 0 does nothing ...
    with pytest.raises(msdr.MsdrError) as e:
        nco.set_osc_channels(5, oi[:2], oq[:2])
    assert e.value.status == msdr.STATUS_ARGUMENT_ERROR
    with pytest.raises(ValueError):
        nco.set_osc_channels(0, oi[:, :100], oq[:, :100])
    for a, b in ((fs4, fs4_control), (nco, nco_control)):
        ga, gb = run(ctx, a, x, B), run(ctx, b, x, B)
        assert np.array_equal(ga, gb)
        assert a.info() == b.info() and PCO not in a.info()["kernel"]                 # ... not even the change of kernel
    for c in range(ch):
        assert np.array_equal(ga[c], orc.chain_q15(x[c], LSB, am, am, mixer=1, osc_i=oi[0], osc_q=oq[0])), c
    for o in (fs4, fs4_control, nco, nco_control):
        o.close()


# ------------------------------------------------------------------------------------------------ 5. HIP graph
def test_graph_made_before_is_refused_one_made_after_replays_and_is_refused_after_the_next_change(ctx, orc):
    rng = np.random.default_rng(5)
    ch, T, L = 10, 2, 128
    taps = np.stack([bw_taps(700.0 + 400.0 * c) for c in range(ch)])
    oi0, oq0 = rows(1, L, seed=8)
    cur_i, cur_q = np.tile(oi0, (ch, 1)), np.tile(oq0, (ch, 1))
    chains = [msdr.Chain(ctx, msdr.ARITH_Q15, ch, taps[0], taps[0], mixer=msdr.MIXER_NCO, mode=USB, osc_i=oi0[0], osc_q=oq0[0]) for _ in range(2)]
    chain, twin = chains                                               # the twin gets every call directly
    for o in chains:
        o.set_taps_channels(0, taps)                                   # (chain_q15pc_kernel: a Q15 chain with a 128-entry table can be captured)
    dxs, dys = [ctx.array((ch, B), np.int16) for _ in range(T)], [ctx.array((ch, B), np.int16) for _ in range(T)]
    states = [{} for _ in range(ch)]

    def check(x, got, tag):
        assert np.array_equal(got, run(ctx, twin, x, B)), tag
        si, sq = at(cur_i, 0, x.shape[1]), at(cur_q, 0, x.shape[1])    # (whole tables per tick: the position is 0 at every tick)
        for c in range(ch):
            assert np.array_equal(got[c], oracle_row(orc, x[c], si[c], sq[c], lambda b: (USB, taps[c], taps[c]), states[c])), (tag, c)

    def replay(g, tag):
        x = rng.integers(-20000, 20001, (ch, T * B)).astype(np.int16)
        for j in range(T):
            dxs[j].upload(x[:, j * B:(j + 1) * B])
        g.launch()
        check(x, np.concatenate([dys[j].download() for j in range(T)], axis=1), tag)

    def direct(tag):
        x = rng.integers(-20000, 20001, (ch, T * B)).astype(np.int16)
        check(x, run(ctx, chain, x, B), tag)

    def retable(first, count, seed):
        nonlocal cur_i, cur_q
        ni, nq = rows(count, L, seed=seed)
        for o in chains:
            o.set_osc_channels(first, ni, nq)
        cur_i, cur_q = cur_i.copy(), cur_q.copy()
        cur_i[first:first + count], cur_q[first:first + count] = ni, nq

    def refused(g):
        with pytest.raises(msdr.MsdrError) as e:
            g.launch()
        assert e.value.status == msdr.STATUS_ARGUMENT_ERROR
        g.close()

    g = chain.graph(dxs, dys, B)
    replay(g, "shared table")
    retable(0, ch, 1)
    refused(g)                                                         # its launches read ONE table
    with pytest.raises(msdr.MsdrError):                                # a pending generation: not capturable
        chain.graph(dxs, dys, B)
    direct("first ticks with rows")                                    # 256 samples: the history has turned over
    assert chain.info()["kernel"].startswith(PCO)
    g = chain.graph(dxs, dys, B)
    replay(g, "replay 1")
    replay(g, "replay 2")
    retable(2, 5, 2)
    refused(g)                                                         # the change made a generation the captured launches know nothing of
    direct("after the change")
    g = chain.graph(dxs, dys, B)
    replay(g, "replay 3")
    one = rows(1, L, seed=6)
    for o in chains:
        o.set_osc(one[0][0], one[1][0])
    cur_i, cur_q = np.tile(one[0], (ch, 1)), np.tile(one[1], (ch, 1))
    refused(g)
    direct("after set_osc")
    assert chain.info()["kernel"].startswith(PCO)
    for o in chains:
        o.close()
