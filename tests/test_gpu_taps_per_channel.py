"""Per-receiver FIR coefficients (Q15): the reference keeps filterBandwidth per station (stations.h:10-16) and calc_demod_filter() rewrites
FIR_AM_coeffs for each value (Minimal-SDR.ino:221-223).  msdr_chain_set_taps_channels / msdr_fir_q15_set_coeffs_channels give single
channels coefficient rows of their own; chain_q15pc_kernel reads every channel's own rows.

The oracle (orclib.Oracle.chain_q15 / fir_q15_blocks take the coefficient arrays per call and keep state outside the configuration) is
evaluated one channel at a time with that channel's coefficients.  Everything is int16 and bit-exact: np.array_equal, no tolerance."""
import numpy as np
import pytest

import orclib
from gpuhelp import ctx, msdr  # noqa: F401

pytestmark = pytest.mark.gpu
B = 128
NT = 102
CORR = orclib.AUDIO_SAMPLE_RATE_EXACT / 24000.0
PC = "chain_q15pc_kernel"


def bw_taps(bw, n=NT):
    """calc_demod_filter(): calc_FIR_coeffs(FIR_AM_coeffs, numTaps, filter_bandwidth, 70, 0, 0.0, 24000)"""
    return msdr.calc_fir_coeffs(n, float(bw), 70.0, 0, 0.0, 24000.0)[:n].copy()


def bank_taps(ch, lo=125.0, hi=5000.0):
    """ch distinct bandwidths of the menu's range (UI.cpp:332-345: steps of 25 Hz from 125 to 5000 Hz)"""
    bws = np.round(np.linspace(lo, hi, ch) / 25.0) * 25.0 if ch <= 196 else lo + (np.arange(ch) % 196) * 25.0
    return np.stack([bw_taps(b) for b in bws])


def pad(t, n=NT):
    return np.concatenate([np.zeros(n - t.size, np.int16), np.asarray(t, np.int16)])


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


def lowpass():
    return msdr.biquad_design(msdr.BQ_LOWPASS, np.float32(5400.0 * CORR), 0.54)


def notch(c):
    return msdr.biquad_design(msdr.BQ_NOTCH, np.float32((3000.0 + 0.37 * c) * CORR), 15.0)


# ------------------------------------------------------------------------------------------------ 1. every channel its own bandwidth
def test_64_channels_64_bandwidths_ticks_and_one_long_call(ctx, orc):
    rng = np.random.default_rng(1)
    ch = 64
    taps = bank_taps(ch)
    assert len({t.tobytes() for t in taps}) == ch                      # 64 distinct filters: more than MSDR_MAX_TAPSETS
    x = rng.integers(-20000, 20001, (ch, 12 * B)).astype(np.int16)
    outs = []
    for step in (B, 12 * B):
        chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, taps[0], taps[0], mode=orclib.AM)
        chain.set_taps_channels(0, taps)
        outs.append(run(ctx, chain, x, step))
        assert chain.info()["kernel"].startswith(PC)
    for c in range(ch):
        assert np.array_equal(outs[0][c], orc.chain_q15(x[c], orclib.AM, taps[c], taps[c])), c
    assert np.array_equal(outs[0], outs[1])


# ------------------------------------------------------------------------------------------------ 2. mixed bank
def test_mixed_bank_shared_sets_beside_own_taps(ctx, orc, golden):
    rng = np.random.default_rng(2)
    ch = 70
    am = bw_taps(2400.0)
    sets_i = [am, pad(golden["taps/FIR_SSB_I_coeffs"]), pad(golden["taps/FIR_CW_I_coeffs"])]
    sets_q = [am, pad(golden["taps/FIR_SSB_Q_coeffs"]), pad(golden["taps/FIR_CW_Q_coeffs"])]
    modes = np.array([(orclib.AM, orclib.LSB, orclib.USB, orclib.CW, orclib.AM)[c % 5] for c in range(ch)], np.int32)
    tapsets = np.array([(0, 1, 1, 2, 0)[c % 5] for c in range(ch)], np.int32)
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, sets_i, sets_q, modes=modes, tapsets=tapsets)
    own = {c: bw_taps(300.0 + 50.0 * c) for c in range(ch) if c % 5 == 0}          # the AM channels c % 5 == 0 get their own; c % 5 == 4 stay shared
    for c, t in own.items():
        chain.set_taps_channels(c, t[None, :])
    states = {c: {} for c in range(ch)}

    def coeffs(c):
        return (own[c], own[c]) if c in own else (sets_i[tapsets[c]], sets_q[tapsets[c]])

    def tick(k):
        x = rng.integers(-20000, 20001, (ch, 3 * B)).astype(np.int16)
        got = run(ctx, chain, x, B if k % 2 == 0 else None)
        assert chain.info()["kernel"].startswith(PC)
        for c in range(ch):
            ci, cq = coeffs(c)
            assert np.array_equal(got[c], orc.chain_q15(x[c], int(modes[c]), ci, cq, state=states[c])), (k, c)

    tick(0)
    # set_taps(tapset) changes the channels still on that tap set only
    am2 = bw_taps(1800.0)
    chain.set_taps(0, am2, am2)
    sets_i[0] = sets_q[0] = am2
    tick(1)
    ssb2_i, ssb2_q = pad(golden["taps/FIR_CW_I_coeffs"]), pad(golden["taps/FIR_CW_Q_coeffs"])
    chain.set_taps(1, ssb2_i, ssb2_q)
    sets_i[1], sets_q[1] = ssb2_i, ssb2_q
    tick(2)
    # set_mode returns one channel to a shared set: its own taps are dropped
    chain.set_mode(10, orclib.USB, 1)
    modes[10], tapsets[10] = orclib.USB, 1
    del own[10]
    chain.set_mode(5, orclib.AM, 0)
    del own[5]
    tick(3)
    chain.set_taps_channels(10, bw_taps(700.0)[None, :])             # and gets new ones again
    own[10] = bw_taps(700.0)
    tick(4)


# ------------------------------------------------------------------------------------------------ 3. change-over in mid-stream
@pytest.mark.parametrize("step", [B, None])
def test_change_over_mid_stream(ctx, orc, step):
    rng = np.random.default_rng(3)
    ch, k = 64, 3
    am = bw_taps(2400.0)
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, am, am, mode=orclib.AM)
    cur = [am] * ch
    states = [{} for _ in range(ch)]

    def ticks(tag):
        x = rng.integers(-20000, 20001, (ch, k * B)).astype(np.int16)
        got = run(ctx, chain, x, step)
        for c in range(ch):
            assert np.array_equal(got[c], orc.chain_q15(x[c], orclib.AM, cur[c], cur[c], state=states[c])), (tag, c)

    ticks(0)
    uniform = chain.info()["kernel"]
    assert not uniform.startswith(PC) and uniform.startswith("chain_q15m")
    t1 = bank_taps(ch)
    chain.set_taps_channels(0, t1)
    cur = list(t1)
    ticks(1)
    assert chain.info()["kernel"].startswith(PC)
    t2 = np.stack([bw_taps(4000.0 - 30.0 * c) for c in range(20, 41)])
    chain.set_taps_channels(20, t2)
    for c in range(20, 41):
        cur[c] = t2[c - 20]
    ticks(2)
    assert chain.info()["kernel"].startswith(PC)


# ------------------------------------------------------------------------------------------------ 4. arithmetic corners
def test_arithmetic_corners_next_to_ordinary_channels(ctx, orc, golden):
    rng = np.random.default_rng(4)
    ch, n = 16, 6 * B
    am = bw_taps(2400.0)
    rows = [bw_taps(500.0 + 200.0 * c) for c in range(ch)]
    rows[1] = pad(golden["fir/taps_wrap8"])                           # the accumulator-wrap tap set
    rows[3] = np.full(NT, 32767, np.int16)
    rows[5] = np.full(NT, -32768, np.int16)
    rows[7] = np.zeros(NT, np.int16)
    rows[9] = np.full(NT, 32767, np.int16)
    rows[11] = np.full(NT, -32768, np.int16)
    rows = np.stack(rows)
    x = rng.integers(-32768, 32768, (ch, n)).astype(np.int16)
    t = np.arange(n)
    x[1] = np.where(t % 4 < 2, 32767, -32768)                         # after the Fs/4 signs every product has the same sign
    x[3] = np.where(t % 4 < 2, 32767, -32768)
    x[5] = np.where(t % 4 < 2, -32768, 32767)
    x[7] = 32767
    x[9] = -32768                                                     # the mixer's wrapping negate, the envelope's wrapping sum
    x[11] = np.where((t // 40) % 2, 32767, -32768)
    for mode in (orclib.AM, orclib.LSB):
        for step in (B, None):
            chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, am, am, mode=mode)
            chain.set_taps_channels(0, rows)
            got = run(ctx, chain, x, step)
            for c in range(ch):
                assert np.array_equal(got[c], orc.chain_q15(x[c], mode, rows[c], rows[c])), (mode, step, c)


# ------------------------------------------------------------------------------------------------ 5. NCO mixer, arm_sqrt_q31, coeffs_q == NULL
@pytest.mark.parametrize("period", [128, 4])
@pytest.mark.parametrize("sqrt_kind", [orclib.SQRT_F32, orclib.SQRT_Q31])
def test_nco_mixer_and_both_square_roots(ctx, orc, golden, period, sqrt_kind):
    rng = np.random.default_rng(50 + period + sqrt_kind)
    ch = 12
    k = np.arange(B)
    cyc = 4.0 if period == 4 else 128.0 / 3.0                          # 3 cycles: a table whose only period is its 128 entries
    oi = np.round(32767 * np.sin(2 * np.pi * k / cyc)).astype(np.int16)
    oq = np.round(32767 * np.cos(2 * np.pi * k / cyc)).astype(np.int16)
    modes = np.array([(orclib.AM, orclib.LSB, orclib.USB, orclib.CW)[c % 4] for c in range(ch)], np.int32)
    ti = np.stack([bw_taps(400.0 + 300.0 * c) if modes[c] in (orclib.AM, orclib.CW) else pad(golden["taps/FIR_SSB_I_coeffs"]) for c in range(ch)])
    tq = np.stack([ti[c] if modes[c] in (orclib.AM, orclib.CW) else pad(golden["taps/FIR_SSB_Q_coeffs"]) for c in range(ch)])
    x = rng.integers(-30000, 30001, (ch, 6 * B)).astype(np.int16)
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, ti[0], ti[0], mixer=msdr.MIXER_NCO, modes=modes, osc_i=oi[:period] if period == 4 else oi,
                       osc_q=oq[:period] if period == 4 else oq, sqrt_kind=sqrt_kind)
    chain.set_taps_channels(0, ti, tq)
    got = np.concatenate([run(ctx, chain, x[:, :3 * B], B), run(ctx, chain, x[:, 3 * B:])], axis=1)
    assert chain.info()["kernel"].startswith(PC)
    for c in range(ch):
        want = orc.chain_q15(x[c], int(modes[c]), ti[c], tq[c], mixer=1, osc_i=oi, osc_q=oq, sqrt_kind=sqrt_kind)
        assert np.array_equal(got[c], want), c


def test_null_coeffs_q_is_the_same_array_twice(ctx):
    rng = np.random.default_rng(55)
    ch = 9
    taps = bank_taps(ch)
    x = rng.integers(-20000, 20001, (ch, 4 * B)).astype(np.int16)
    am = bw_taps(2400.0)
    a = msdr.Chain(ctx, msdr.ARITH_Q15, ch, am, am, mode=orclib.LSB)
    b = msdr.Chain(ctx, msdr.ARITH_Q15, ch, am, am, mode=orclib.LSB)
    a.set_taps_channels(0, taps)
    b.set_taps_channels(0, taps, taps)
    assert np.array_equal(run(ctx, a, x, B), run(ctx, b, x, B))


# ------------------------------------------------------------------------------------------------ 6. the passes behind the kernel
@pytest.mark.parametrize("step", [B, 4 * B])
def test_nodes_anr_and_pll_behind_the_kernel(ctx, orc, step):
    rng = np.random.default_rng(6)
    ch, n = 66, 8 * B
    t = np.arange(n)
    x = np.stack([(9000 * (1 + 0.5 * np.sin(2 * np.pi * 400 * t / 24000)) * np.cos(2 * np.pi * 6000 * t / 24000 + c)
                   + 1500 * np.cos(2 * np.pi * 7000 * t / 24000) + rng.integers(-100, 101, n)).astype(np.int16) for c in range(ch)])
    taps = bank_taps(ch, 1000.0, 5000.0)
    modes = np.array([orclib.SYNCAM if c % 3 == 0 else orclib.AM for c in range(ch)], np.int32)
    anr_on = np.array([(0, 1, 2, 0, 0)[c % 5] for c in range(ch)], np.int32)
    lp = lowpass()
    rows = {c: notch(c) for c in range(ch) if c % 2}                   # per-channel notch on the odd channels, the uniform one elsewhere
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, taps[0], taps[0], modes=modes, biquad_nodes=[[lp], [notch(0)]], flags=msdr.CHAIN_SYNCAM_PLL)
    chain.set_anr(anr_on)
    for c, r in rows.items():
        chain.set_node_coefficients_channels(1, c, 0, r[None, :])
    chain.set_taps_channels(0, taps)
    got = run(ctx, chain, x, step)
    assert chain.info()["kernel"].startswith(PC)
    for c in range(ch):
        audio, i_f, q_f = orc.chain_q15(x[c], orclib.AM, taps[c], taps[c], want_iq=True)
        if modes[c] == orclib.SYNCAM:
            audio = orc.syncam_q15(orc.syncam_new(), i_f, q_f)
        audio = orc.anr_q15(orc.anr_new(), anr_on[c], audio)
        audio = orc.biquad_teensy_update(orc.biquad_teensy_new([lp]), audio)
        want = orc.biquad_teensy_update(orc.biquad_teensy_new([rows.get(c, notch(0))]), audio)
        assert np.array_equal(got[c], want), c


# ------------------------------------------------------------------------------------------------ 7. block lengths and channel counts
@pytest.mark.parametrize("n", [32, 64, 256, 512, 1000, 2 ** 14])
def test_block_lengths(ctx, orc, n):
    rng = np.random.default_rng(700 + n)
    ch = 10
    calls = {32: 8, 64: 6, 256: 3, 512: 3, 1000: 16, 2 ** 14: 2}[n]   # (the oracle walks whole 128-sample blocks: calls * n is a multiple of 128)
    taps = bank_taps(ch)
    modes = np.array([(orclib.AM, orclib.LSB)[c % 2] for c in range(ch)], np.int32)
    x = rng.integers(-20000, 20001, (ch, calls * n)).astype(np.int16)
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, taps[0], taps[0], modes=modes)
    chain.set_taps_channels(0, taps)
    got = run(ctx, chain, x, n)
    for c in range(ch):
        assert np.array_equal(got[c], orc.chain_q15(x[c], int(modes[c]), taps[c], taps[c])), c


@pytest.mark.parametrize("ch", [1, 3, 63, 65, 4096])
def test_channel_counts(ctx, orc, ch):
    rng = np.random.default_rng(800 + ch)
    taps = bank_taps(ch)
    x = rng.integers(-20000, 20001, (ch, 4 * B)).astype(np.int16)
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, taps[0], taps[0], mode=orclib.AM)
    chain.set_taps_channels(0, taps)
    got = np.concatenate([run(ctx, chain, x[:, :2 * B], B), run(ctx, chain, x[:, 2 * B:])], axis=1)
    # 4096 channels: every 61st channel plus the first and the last 8
    check = range(ch) if ch < 4096 else sorted(set(range(0, ch, 61)) | set(range(8)) | set(range(ch - 8, ch)))
    for c in check:
        assert np.array_equal(got[c], orc.chain_q15(x[c], orclib.AM, taps[c], taps[c])), c


# ------------------------------------------------------------------------------------------------ 8. what keeps the taps; argument errors
def test_init_fir_reset_set_osc_keep_the_taps(ctx, orc):
    rng = np.random.default_rng(8)
    ch = 20
    k = np.arange(B)
    tabs = [(np.round(32767 * np.sin(2 * np.pi * k * f / 128)).astype(np.int16), np.round(32767 * np.cos(2 * np.pi * k * f / 128)).astype(np.int16)) for f in (32, 16)]
    taps = bank_taps(ch)
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, taps[0], taps[0], mixer=msdr.MIXER_NCO, mode=orclib.LSB, osc_i=tabs[0][0], osc_q=tabs[0][1])
    chain.set_taps_channels(0, taps)
    states = [{} for _ in range(ch)]
    cur = 0
    for j in range(5):
        if j == 1:
            chain.init_fir()
            states = [{} for _ in range(ch)]
        if j == 2:
            chain.reset()
            states = [{} for _ in range(ch)]
        if j == 3:
            chain.set_osc(*tabs[1])
            cur = 1
        x = rng.integers(-20000, 20001, (ch, 3 * B)).astype(np.int16)
        got = run(ctx, chain, x, B if j != 4 else None)
        assert chain.info()["kernel"].startswith(PC)
        for c in range(ch):
            want = orc.chain_q15(x[c], orclib.LSB, taps[c], taps[c], mixer=1, osc_i=tabs[cur][0], osc_q=tabs[cur][1], state=states[c])
            assert np.array_equal(got[c], want), (j, c)


def test_argument_errors_and_count_zero(ctx, orc):
    rng = np.random.default_rng(81)
    ch = 6
    am = bw_taps(2400.0)
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, am, am, mode=orclib.AM)
    rows = bank_taps(3)
    with pytest.raises(msdr.MsdrError) as e:
        chain.set_taps_channels(4, rows)                              # 4 .. 6 of 6
    assert e.value.status == msdr.STATUS_ARGUMENT_ERROR
    with pytest.raises(msdr.MsdrError):
        chain.set_taps_channels(6, rows[:1])
    assert ctx.lib.msdr_chain_set_taps_channels(chain.h, 0, 2, None, None) == msdr.STATUS_ARGUMENT_ERROR
    assert ctx.lib.msdr_chain_set_taps_channels(chain.h, 0, 0, None, None) == 0         # count == 0 does nothing ...
    chain.set_taps_channels(0, np.zeros((0, NT), np.int16))
    x = rng.integers(-20000, 20001, (ch, 2 * B)).astype(np.int16)
    got = run(ctx, chain, x, B)
    assert not chain.info()["kernel"].startswith(PC)                 # ... not even the change of kernel
    for c in range(ch):
        assert np.array_equal(got[c], orc.chain_q15(x[c], orclib.AM, am, am)), c
    with pytest.raises(ValueError):
        chain.set_taps_channels(0, np.zeros((2, NT - 2), np.int16))
    lp = np.ones(NT, np.float32) / NT
    f = msdr.Chain(ctx, msdr.ARITH_F32, 4, lp, lp, mixer=msdr.MIXER_FS4, mode=orclib.AM)
    with pytest.raises(msdr.MsdrError) as e:
        f.set_taps_channels(0, rows)
    assert e.value.status == msdr.STATUS_ARGUMENT_ERROR
    assert "Q15" in str(e.value)


# ------------------------------------------------------------------------------------------------ 9. HIP graph
def test_graph_made_before_is_refused_and_one_made_after_replays_bit_exactly(ctx, orc):
    rng = np.random.default_rng(9)
    ch, T = 64, 2
    am = bw_taps(2400.0)
    lp = lowpass()
    taps = bank_taps(ch)
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, am, am, mode=orclib.AM, biquad_nodes=[[lp], [notch(0)]])
    dxs, dys = [ctx.array((ch, B), np.int16) for _ in range(T)], [ctx.array((ch, B), np.int16) for _ in range(T)]
    x = rng.integers(-20000, 20001, (ch, 4 * T * B)).astype(np.int16)
    got, o = np.empty_like(x), 0

    def replay(g):
        nonlocal o
        for k in range(T):
            dxs[k].upload(x[:, o + B * k:o + B * (k + 1)])
        g.launch()
        for k in range(T):
            got[:, o + B * k:o + B * (k + 1)] = dys[k].download()
        o += B * T

    g = chain.graph(dxs, dys, B)
    replay(g)
    chain.set_taps_channels(0, taps)
    with pytest.raises(msdr.MsdrError) as e:                          # its launches share tap sets between channels
        g.launch()
    assert e.value.status == msdr.STATUS_ARGUMENT_ERROR
    g.close()
    g = chain.graph(dxs, dys, B)                                      # chain_q15pc_kernel + node kernel + history kernel
    replay(g)
    replay(g)
    t2 = np.stack([bw_taps(900.0 + 10.0 * c) for c in range(8)])
    chain.set_taps_channels(3, t2)                                    # the captured launches read the table: the graph stays valid
    replay(g)
    g.close()
    assert o == x.shape[1]
    for c in range(ch):
        nodes, st = [orc.biquad_teensy_new([lp]), orc.biquad_teensy_new([notch(0)])], {}
        w1 = orc.chain_q15(x[c, :T * B], orclib.AM, am, am, biquads=nodes, state=st)
        w2 = orc.chain_q15(x[c, T * B:3 * T * B], orclib.AM, taps[c], taps[c], biquads=nodes, state=st)
        tc = t2[c - 3] if 3 <= c < 11 else taps[c]
        w3 = orc.chain_q15(x[c, 3 * T * B:], orclib.AM, tc, tc, biquads=nodes, state=st)
        assert np.array_equal(got[c], np.concatenate([w1, w2, w3])), c


def test_a_graph_is_refused_after_a_rebuild_on_a_chain_without_matrix_core_tables(ctx, orc):
    """MSDR_CHAIN_NO_MFMA: no matrix-core tables, so before per-channel taps no graph could be made of such a chain at all.  Its captured
    launches point at the mode array and the oscillator table of the chain as it was: set_taps / set_osc rebuild both, reset moves the
    mixer's position -- each must refuse the replay (nothing enqueued), and a graph made again replays bit-exactly."""
    rng = np.random.default_rng(91)
    ch, T = 12, 2
    k = np.arange(B)
    tabs = [(np.round(32767 * np.sin(2 * np.pi * k * f / 128)).astype(np.int16), np.round(32767 * np.cos(2 * np.pi * k * f / 128)).astype(np.int16)) for f in (32, 16)]
    am, am2 = bw_taps(2400.0), bw_taps(1500.0)
    taps = bank_taps(ch)
    own = ch // 2                                                     # channels 0 .. 5 their own taps, 6 .. 11 on the shared set
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, am, am, mixer=msdr.MIXER_NCO, mode=orclib.LSB, osc_i=tabs[0][0], osc_q=tabs[0][1], flags=msdr.CHAIN_NO_MFMA)
    chain.set_taps_channels(0, taps[:own])
    dxs, dys = [ctx.array((ch, B), np.int16) for _ in range(T)], [ctx.array((ch, B), np.int16) for _ in range(T)]
    states = [{} for _ in range(ch)]
    shared, cur = am, 0

    def check(x, got, tag):
        for c in range(ch):
            t = taps[c] if c < own else shared
            want = orc.chain_q15(x[c], orclib.LSB, t, t, mixer=1, osc_i=tabs[cur][0], osc_q=tabs[cur][1], state=states[c])
            assert np.array_equal(got[c], want), (tag, c)

    def replay(g, tag):
        x = rng.integers(-20000, 20001, (ch, T * B)).astype(np.int16)
        for j in range(T):
            dxs[j].upload(x[:, j * B:(j + 1) * B])
        g.launch()
        check(x, np.concatenate([dys[j].download() for j in range(T)], axis=1), tag)

    def direct(blocks, tag):
        x = rng.integers(-20000, 20001, (ch, blocks * B)).astype(np.int16)
        check(x, run(ctx, chain, x, B), tag)

    def refused(g):
        with pytest.raises(msdr.MsdrError) as e:
            g.launch()
        assert e.value.status == msdr.STATUS_ARGUMENT_ERROR
        g.close()

    g = chain.graph(dxs, dys, B)
    replay(g, "first")
    assert chain.info()["kernel"].startswith(PC)
    chain.set_taps(0, am2, am2)                                       # a rebuild: the old mode array and oscillator table are freed
    shared = am2
    refused(g)
    g = chain.graph(dxs, dys, B)
    replay(g, "after set_taps")
    chain.set_osc(*tabs[1])
    cur = 1
    refused(g)
    with pytest.raises(msdr.MsdrError):                               # the history still holds samples of the earlier table: not capturable
        chain.graph(dxs, dys, B)
    direct(2, "after set_osc")                                       # 256 samples: the 105-sample history has turned over
    g = chain.graph(dxs, dys, B)
    replay(g, "new table")
    chain.reset()
    states = [{} for _ in range(ch)]
    refused(g)
    g = chain.graph(dxs, dys, B)
    replay(g, "after reset")
    g.close()


def test_set_anr_and_the_node_setters_after_the_first_call_keep_the_taps(ctx, orc):
    rng = np.random.default_rng(92)
    ch = 10
    taps = bank_taps(ch, 1000.0, 5000.0)
    lp, lp2 = lowpass(), msdr.biquad_design(msdr.BQ_LOWPASS, np.float32(4000.0 * CORR), 0.7)
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, taps[0], taps[0], mode=orclib.AM, biquad_nodes=[[lp], [notch(0)]])
    chain.set_taps_channels(0, taps)
    anr_on = np.array([(0, 1, 2)[c % 3] for c in range(ch)], np.int32)
    chain.set_anr(anr_on)                                             # all three AFTER the first per-channel call
    chain.set_node_coefficients(0, 0, lp2)
    rows = np.stack([notch(7 * c) for c in range(ch)])
    chain.set_node_coefficients_channels(1, 0, 0, rows)
    t = np.arange(6 * B)
    x = np.stack([(9000 * (1 + 0.5 * np.sin(2 * np.pi * 400 * t / 24000)) * np.cos(2 * np.pi * 6000 * t / 24000 + c)
                   + rng.integers(-100, 101, t.size)).astype(np.int16) for c in range(ch)])
    got = run(ctx, chain, x, B)
    assert chain.info()["kernel"].startswith(PC)
    for c in range(ch):
        audio = orc.chain_q15(x[c], orclib.AM, taps[c], taps[c])
        audio = orc.anr_q15(orc.anr_new(), anr_on[c], audio)
        audio = orc.biquad_teensy_update(orc.biquad_teensy_new([lp2]), audio)
        assert np.array_equal(got[c], orc.biquad_teensy_update(orc.biquad_teensy_new([rows[c]]), audio)), c


# ------------------------------------------------------------------------------------------------ 10. the arm_fir_fast_q15 stage
def fir_expect(orc, segs, x, block):
    """one channel's stream under coefficient arrays that change between calls: segs = [(first sample, coefficients), ...].  arm_fir_fast_q15
    keeps numTaps - 1 samples of state, so a fresh instance fed the numTaps - 1 inputs before a stretch first is the carried one."""
    out = []
    for j, (a, cf) in enumerate(segs):
        b = segs[j + 1][0] if j + 1 < len(segs) else x.size
        ntaps = cf.size
        pre = max(0, a - (ntaps - 1))
        z = ntaps + (-(ntaps + a - pre)) % block                      # (so that the stretch under test starts on a block boundary)
        st, y = orc.fir_q15_blocks(cf, np.concatenate([np.zeros(z, np.int16), x[pre:b]]), block)
        assert st == 0
        out.append(y[z + (a - pre):])
    return np.concatenate(out)


@pytest.mark.parametrize("block", [1, 2, 127, 128, 129, 256])
def test_fir_stage_with_per_channel_coefficients(ctx, orc, block):
    rng = np.random.default_rng(1000 + block)
    ch = 40
    for ntaps in sorted({2, 278} | {int(v) for v in 2 * rng.integers(1, 140, 3)}):
        rows = rng.integers(-32768, 32768, (ch, ntaps)).astype(np.int16)
        rows[0] = 32767
        rows[1] = -32768
        shared = rng.integers(-3000, 3001, ntaps).astype(np.int16)
        shared2 = rng.integers(-32768, 32768, ntaps).astype(np.int16)
        S = msdr.FirQ15(ctx, shared, ch)
        calls = 8
        x = rng.integers(-32768, 32768, (ch, calls * block)).astype(np.int16)
        x[0] = 32767
        x[1] = -32768
        got = np.empty_like(x)
        for k in range(calls):
            if k == 2:                                                # mid-stream: channels 0 .. 29 only; 30 .. 39 keep the shared coefficients
                S.set_coeffs_channels(0, rows[:30])
            if k == 4:                                                # the rest in a second call
                S.set_coeffs_channels(30, rows[30:])
            if k == 6:                                                # the uniform setter on a per-channel instance writes ALL channels
                S.set_coeffs(shared2)
            dx, dy = ctx.to_device(np.ascontiguousarray(x[:, k * block:(k + 1) * block])), ctx.array((ch, block), np.int16)
            S.process(dx, dy, block)
            got[:, k * block:(k + 1) * block] = dy.download()
        for c in range(ch):
            segs = [(0, shared), (2 * block if c < 30 else 4 * block, rows[c]), (6 * block, shared2)]
            assert np.array_equal(got[c], fir_expect(orc, segs, x[c], block)), (ntaps, c)
        with pytest.raises(msdr.MsdrError):
            S.set_coeffs_channels(39, rows[:2])
        S.set_coeffs_channels(0, rows[:0])


def test_fir_stage_refuses_filters_the_kernel_cannot_hold(ctx, orc):
    """more than 10 576 taps: a channel's window does not fit the kernel's LDS -- the setter refuses and the instance goes on as it was"""
    rng = np.random.default_rng(93)
    ntaps, n = 10600, 256
    cf = rng.integers(-300, 301, ntaps).astype(np.int16)
    S = msdr.FirQ15(ctx, cf, 2)
    with pytest.raises(msdr.MsdrError) as e:
        S.set_coeffs_channels(0, np.stack([cf, cf]))
    assert e.value.status == msdr.STATUS_ARGUMENT_ERROR and "taps" in str(e.value)
    x = rng.integers(-32768, 32768, (2, n)).astype(np.int16)
    dx, dy = ctx.to_device(x), ctx.array((2, n), np.int16)
    S.process(dx, dy, n)
    got = dy.download()
    for c in range(2):
        st, y = orc.fir_q15_blocks(cf, x[c], n)
        assert st == 0 and np.array_equal(got[c], y), c
