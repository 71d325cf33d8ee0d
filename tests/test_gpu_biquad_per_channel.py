"""Per-receiver AudioFilterBiquad coefficients: tune() ends with biquad2_dac.setNotch(0, pdb_freq_actual / 8.0 * CORR_FACT, 15.0)
(Minimal-SDR.ino:356) and pdb_freq_actual belongs to the frequency THAT receiver is tuned to (:343-352), so two receivers of a bank have two
notches.  msdr_biquad_q15_set_coefficients_channels / msdr_chain_set_node_coefficients_channels write single channels' records and
biquad_teensy_pc_kernel reads every lane's own coefficients and stage count.

The oracle (orc_biquad_teensy_init / set_coefficients / update, and the chain oracle over such nodes) is run once per channel with that
channel's coefficients.  Everything is int16 and bit-exact: np.array_equal, no tolerance."""
import ctypes as C

import numpy as np
import pytest

import orclib
from gpuhelp import ctx, msdr  # noqa: F401

pytestmark = pytest.mark.gpu
B = 128
CORR = orclib.AUDIO_SAMPLE_RATE_EXACT / 24000.0
FLAG = np.int32(-2 ** 31)


def notch(ch, base=3000.0):
    """tune()'s notch of receiver ch: every receiver a slightly different pdb_freq_actual / 8"""
    return msdr.biquad_design(msdr.BQ_NOTCH, np.float32((base + 0.37 * ch) * CORR), 15.0)


def lowpass(f=5400.0, q=0.54):
    return msdr.biquad_design(msdr.BQ_LOWPASS, np.float32(f * CORR), q)


def orc_set(orc, b, stage, coef):
    orc.lib.orc_biquad_teensy_set_coefficients(C.byref(b), C.c_uint32(stage), orclib._ptr(np.ascontiguousarray(coef, np.int32)))


def signal(rng, ch, n):
    """noise with full-scale +32767 / -32768 stretches: the saturation and the 14-bit residue both at work"""
    x = rng.integers(-32768, 32768, (ch, n)).astype(np.int16)
    for c in range(ch):
        k = int(rng.integers(0, max(1, n - 8)))
        m = int(rng.integers(2, 40))
        x[c, k:k + m] = 32767 if c % 2 else -32768
        if n >= 64:
            x[c, n // 2:n // 2 + 9] = -32768 if c % 2 else 32767
    return x


def check_definitions(S, nodes, channels):
    """words 0-4 of every stage and the flag bits, as the oracle's definition[] holds them"""
    for c in channels:
        got, want = S.definition(c), np.frombuffer(nodes[c], np.int32)
        for s in range(4):
            assert np.array_equal(got[8 * s:8 * s + 5], want[8 * s:8 * s + 5]), (c, s)
            assert (got[8 * s + 7] & FLAG) == (want[8 * s + 7] & FLAG), (c, s)


def run_update(ctx, S, x, misalign=False):
    ch, n = x.shape
    if not misalign:
        d = ctx.to_device(x)
        S.update(d, n)
        return d.download()
    flat = ctx.array(ch * n + 8, np.int16)                       # the batch one sample off a 16-byte boundary
    flat.upload(np.concatenate([np.zeros(1, np.int16), x.reshape(-1), np.zeros(7, np.int16)]))
    S.update(flat.offset(2), n)
    return flat.download()[1:1 + ch * n].reshape(ch, n)


# ------------------------------------------------------------------------------------------------ 3. the stage
@pytest.mark.parametrize("channels", [1, 5, 64, 70, 256])
@pytest.mark.parametrize("block", [2, 30, 128, 130, 1024])
def test_every_channel_its_own_notch(ctx, orc, channels, block):
    rng = np.random.default_rng(1000 * channels + block)
    coefs = np.stack([notch(c) for c in range(channels)])
    S = msdr.BiquadQ15(ctx, channels)
    S.set_coefficients_channels(0, 0, coefs)
    nodes = [orc.biquad_teensy_new([coefs[c]]) for c in range(channels)]
    for call in range(3):                                        # state carried from call to call
        x = signal(rng, channels, block)
        got = run_update(ctx, S, x, misalign=(call == 1))
        assert S.last_kernel() == "biquad_teensy_pc_kernel<1>"
        for c in range(channels):
            assert np.array_equal(got[c], orc.biquad_teensy_update(nodes[c], x[c])), (call, c)
    check_definitions(S, nodes, range(channels))


@pytest.mark.parametrize("channels,block", [(64, 128), (70, 130), (256, 1024), (5, 30)])
def test_mixed_stage_counts_inside_one_wave(ctx, orc, channels, block):
    """channel c runs 1 + c % 4 stages: the lanes of one wave run 1, 2, 3 and 4 stages side by side"""
    rng = np.random.default_rng(77 + channels)
    kinds = [lambda c: lowpass(4000.0 + 3 * c, 0.6), lambda c: notch(c), lambda c: lowpass(5000.0 - c, 0.9), lambda c: notch(c, 1500.0)]
    S = msdr.BiquadQ15(ctx, channels)
    nodes = [orc.biquad_teensy_new([]) for _ in range(channels)]
    for s in range(4):
        # stage s goes to the channels that have it, in runs of consecutive channels (c % 4 >= s), one call per run
        c = 0
        while c < channels:
            if c % 4 < s:
                c += 1
                continue
            e = c
            while e < channels and e % 4 >= s:
                e += 1
            rows = np.stack([kinds[s](k) for k in range(c, e)])
            S.set_coefficients_channels(c, s, rows)
            for k in range(c, e):
                orc_set(orc, nodes[k], s, rows[k - c])
            c = e
    for call in range(3):
        x = signal(rng, channels, block)
        got = run_update(ctx, S, x)
        assert S.last_kernel() == "biquad_teensy_pc_kernel<1>"
        for c in range(channels):
            assert np.array_equal(got[c], orc.biquad_teensy_update(nodes[c], x[c])), (call, c)
    check_definitions(S, nodes, range(channels))


def test_untouched_channels_pass_nothing_and_arguments_are_checked(ctx, orc):
    """an all-zero record passes nothing (filter_biquad.h:36-39); a range past the end is refused; count 0 and stage >= 4 do nothing"""
    rng = np.random.default_rng(5)
    ch = 70
    S = msdr.BiquadQ15(ctx, ch)
    rows = np.stack([notch(c) for c in range(10, 20)])
    S.set_coefficients_channels(10, 0, rows)
    with pytest.raises(msdr.MsdrError) as e:
        S.set_coefficients_channels(65, 0, rows)                 # 65 .. 74 of 70
    assert e.value.status == msdr.STATUS_ARGUMENT_ERROR
    with pytest.raises(msdr.MsdrError):
        S.set_coefficients_channels(70, 0, rows[:1])
    S.set_coefficients_channels(0, 4, rows)                      # filter_biquad.cpp:86
    S.set_coefficients_channels(0, 0, np.zeros((0, 5), np.int32))
    assert ctx.lib.msdr_biquad_q15_set_coefficients_channels(S.h, 0, 3, 0, None) == msdr.STATUS_ARGUMENT_ERROR
    x = signal(rng, ch, 256)
    got = run_update(ctx, S, x)
    for c in range(ch):
        node = orc.biquad_teensy_new([rows[c - 10]] if 10 <= c < 20 else [])
        assert np.array_equal(got[c], orc.biquad_teensy_update(node, x[c])), c
    assert not got[:10].any() and not got[20:].any()
    assert not S.definition(9)[:5].any() and not S.definition(20)[:5].any()


# ------------------------------------------------------------------------------------------------ 4. equivalence
@pytest.mark.parametrize("channels,block", [(64, 1024), (128, 256),        # biquad_teensy_pipe4_kernel<1> today
                                            (70, 130), (64, 130), (5, 128)])   # biquad_teensy_kernel<1> today
def test_same_coefficients_everywhere_equal_the_uniform_call(ctx, channels, block):
    rng = np.random.default_rng(9 + channels)
    co = notch(0)
    U, P = msdr.BiquadQ15(ctx, channels), msdr.BiquadQ15(ctx, channels)
    U.set_coefficients(0, co)
    P.set_coefficients_channels(0, 0, np.tile(co, (channels, 1)))
    for call in range(3):
        x = signal(rng, channels, block)
        assert np.array_equal(run_update(ctx, U, x), run_update(ctx, P, x)), call
        assert U.last_kernel() == ("biquad_teensy_pipe4_kernel<1,16>" if (channels, block) in ((64, 1024), (128, 256)) else "biquad_teensy_kernel<1>")
        assert P.last_kernel() == "biquad_teensy_pc_kernel<1>"
    for c in (0, channels - 1):
        assert np.array_equal(U.definition(c), P.definition(c)), c


# ------------------------------------------------------------------------------------------------ 5. hand-over
@pytest.mark.parametrize("channels,block", [(64, 128), (70, 130), (256, 1024)])
def test_hand_over_from_the_uniform_kernels_mid_stream(ctx, orc, channels, block):
    """two blocks uniformly, one channel range re-notched, two more blocks: history kept, residue cleared (filter_biquad.cpp:95-98)"""
    rng = np.random.default_rng(31 + channels)
    co = notch(0)
    S = msdr.BiquadQ15(ctx, channels)
    S.set_coefficients(0, co)
    nodes = [orc.biquad_teensy_new([co]) for _ in range(channels)]
    lo, hi = channels // 3, channels // 3 + max(1, channels // 2)
    for call in range(4):
        if call == 2:
            rows = np.stack([notch(c, 2500.0) for c in range(lo, hi)])
            S.set_coefficients_channels(lo, 0, rows)
            for c in range(lo, hi):
                orc_set(orc, nodes[c], 0, rows[c - lo])
        x = signal(rng, channels, block)
        got = run_update(ctx, S, x)
        uniform = "biquad_teensy_pipe4_kernel<1,16>" if block % 128 == 0 and channels % 16 == 0 else "biquad_teensy_kernel<1>"
        assert S.last_kernel() == (uniform if call < 2 else "biquad_teensy_pc_kernel<1>"), (call, S.last_kernel())
        for c in range(channels):
            assert np.array_equal(got[c], orc.biquad_teensy_update(nodes[c], x[c])), (call, c)
    check_definitions(S, nodes, range(channels))
    # the uniform setter keeps working on a per-channel instance: it writes all channels
    co2 = lowpass()
    S.set_coefficients(0, co2)
    for c in range(channels):
        orc_set(orc, nodes[c], 0, co2)
    x = signal(rng, channels, block)
    got = run_update(ctx, S, x)
    for c in range(channels):
        assert np.array_equal(got[c], orc.biquad_teensy_update(nodes[c], x[c])), c


# ------------------------------------------------------------------------------------------------ 6. the chain
def _chain_case(ctx, orc, ch, block):
    rng = np.random.default_rng(600 + ch)
    am = orc.calc_fir_coeffs(102, 2400.0)[:102].copy()
    am2 = orc.calc_fir_coeffs(102, 1800.0)[:102].copy()
    lp = lowpass()
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, am, am, mode=orclib.AM, biquad_nodes=[[lp], [notch(0)]])
    rows = np.stack([notch(c) for c in range(ch)])
    chain.set_node_coefficients_channels(1, 0, 0, rows)          # before the first call
    nodes = {c: [orc.biquad_teensy_new([lp]), orc.biquad_teensy_new([rows[c]])] for c in range(ch)}
    states = {c: {} for c in range(ch)}
    lo, hi = ch // 4, ch // 4 + ch // 2
    taps = am
    for k in range(5):
        if k == 1:                                               # a sub-range retuned in mid-stream, node 0 of a few channels too
            sub = np.stack([notch(c, 2700.0) for c in range(lo, hi)])
            chain.set_node_coefficients_channels(1, lo, 0, sub)
            lps = np.stack([lowpass(4000.0 + c) for c in range(3)])
            chain.set_node_coefficients_channels(0, 1, 0, lps)
            for c in range(ch):
                recs = states[c].get("bq", nodes[c])
                if lo <= c < hi:
                    orc_set(orc, recs[1], 0, sub[c - lo])
                if 1 <= c < 4:
                    orc_set(orc, recs[0], 0, lps[c - 1])
        if k == 2:                                               # a rebuild of the chain's tables: no per-channel coefficient is lost
            chain.set_taps(0, am2, am2)
            taps = am2
        if k == 3:                                               # FIR state cleared; the nodes keep coefficients AND history (filter_biquad.cpp:95-97)
            chain.reset()
            for c in range(ch):
                bq = states[c]["bq"]
                states[c] = {"bq": bq}
        if k == 4:
            chain.init_fir()
            for c in range(ch):
                bq = states[c]["bq"]
                states[c] = {"bq": bq}
        x = rng.integers(-20000, 20001, (ch, 3 * B)).astype(np.int16)
        got = np.empty_like(x)
        step = block or x.shape[1]
        for o in range(0, x.shape[1], step):
            dx, dy = ctx.to_device(x[:, o:o + step]), ctx.array((ch, step), np.int16)
            chain.process(dx, dy, step)
            assert chain.node_kernel() == "biquad_teensy_pc_kernel<2>"
            got[:, o:o + step] = dy.download()
        for c in range(ch):
            want = orc.chain_q15(x[c], orclib.AM, taps, taps, biquads=nodes[c], state=states[c])
            assert np.array_equal(got[c], want), (k, c)
    with pytest.raises(msdr.MsdrError):
        chain.set_node_coefficients_channels(2, 0, 0, rows)      # no such node
    with pytest.raises(msdr.MsdrError):
        chain.set_node_coefficients_channels(1, ch - 1, 0, rows[:2])


@pytest.mark.parametrize("channels", [64, 200])
@pytest.mark.parametrize("block", [B, None])
def test_chain_with_per_channel_notches(ctx, orc, channels, block):
    """Fs/4, the 102-tap AM set, both nodes; as 128-sample calls and as single long calls"""
    _chain_case(ctx, orc, channels, block)


def test_fp32_chain_refuses_the_call(ctx):
    lp = np.ones(102, np.float32) / 102
    chain = msdr.Chain(ctx, msdr.ARITH_F32, 4, lp, lp, mixer=msdr.MIXER_FS4, mode=orclib.AM)
    with pytest.raises(msdr.MsdrError) as e:
        chain.set_node_coefficients_channels(0, 0, 0, np.zeros((4, 5), np.int32))
    assert e.value.status == msdr.STATUS_ARGUMENT_ERROR


# ------------------------------------------------------------------------------------------------ 7. HIP graph
def test_graph_made_before_is_refused_and_one_made_after_replays_bit_exactly(ctx, orc):
    rng = np.random.default_rng(7)
    ch, T = 64, 2
    am = orc.calc_fir_coeffs(102, 2400.0)[:102].copy()
    lp = lowpass()
    rows = np.stack([notch(c) for c in range(ch)])

    def make():
        return msdr.Chain(ctx, msdr.ARITH_Q15, ch, am, am, mode=orclib.AM, biquad_nodes=[[lp], [notch(0)]])

    chain, direct = make(), make()
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

    g = chain.graph(dxs, dys, B)                                 # uniform nodes: the fused tick
    assert chain.node_kernel() == "chain_q15mb_kernel"
    replay(g)
    chain.set_node_coefficients_channels(1, 0, 0, rows)
    with pytest.raises(msdr.MsdrError) as e:                     # its launches keep a node's coefficients uniform
        g.launch()
    assert e.value.status == msdr.STATUS_ARGUMENT_ERROR
    g.close()
    g = chain.graph(dxs, dys, B)                                 # demodulator kernel + biquad_teensy_pc_kernel<2>
    assert chain.node_kernel() == "biquad_teensy_pc_kernel<2>"
    for _ in range(3):
        replay(g)
    g.close()
    assert o == x.shape[1]
    # the same stream through direct calls on a second chain
    want = np.empty_like(x)
    for k in range(4 * T):
        if k == T:
            direct.set_node_coefficients_channels(1, 0, 0, rows)
        dx, dy = ctx.to_device(x[:, k * B:(k + 1) * B]), ctx.array((ch, B), np.int16)
        direct.process(dx, dy, B)
        want[:, k * B:(k + 1) * B] = dy.download()
    assert np.array_equal(got, want)
    for c in (0, 17, 63):                                        # and both are the oracle's stream
        nodes, st = [orc.biquad_teensy_new([lp]), orc.biquad_teensy_new([notch(0)])], {}
        w1 = orc.chain_q15(x[c, :T * B], orclib.AM, am, am, biquads=nodes, state=st)
        orc_set(orc, st["bq"][1], 0, rows[c])
        w2 = orc.chain_q15(x[c, T * B:], orclib.AM, am, am, biquads=nodes, state=st)
        assert np.array_equal(got[c], np.concatenate([w1, w2])), c
