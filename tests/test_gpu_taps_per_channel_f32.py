"""Per-receiver FIR coefficients for the fp32 chain: msdr_chain_set_taps_channels_f32 / msdr_fir_f32_set_coeffs_channels give single channels
coefficient rows of their own; chain_f32pc_kernel reads every channel's own rows (plain fp32 FMAs).

Every channel is judged on its own: orclib.Oracle.chain_f32 with that channel's coefficients, `state` carried across calls, through
f32judge.judge -- e_go < 1e-5 and e_gpu <= 2 e_orc + fp32_noise + 1e-6 (level 1: tests/test_f32pc_cases.py holds the cases to that).
float64 references of streams whose coefficients change are pieced together from whole-stream float64 runs of each coefficient set: the FIR
pair has no state but its input history, which is what "the new filter over the old filter's history" means (cases without a cascade)."""
import numpy as np
import pytest

import orclib
from f32judge import judge, truth64
from f32pc_cases import B, FS4, NT, bank_taps, bw_taps, cascade, hilbert_pair, nco128
from gpuhelp import ctx, msdr, rel_rms  # noqa: F401

pytestmark = pytest.mark.gpu
PC = "chain_f32pc_kernel"
AM, LSB, USB, CW, SYNCAM = orclib.AM, orclib.LSB, orclib.USB, orclib.CW, orclib.SYNCAM


def run(ctx, chain, x, step=None, dtype=np.float32):
    ch, n = x.shape
    got = np.empty((ch, n), dtype)
    step = step or n
    for o in range(0, n, step):
        m = min(step, n - o)
        dx, dy = ctx.to_device(np.ascontiguousarray(x[:, o:o + m])), ctx.array((ch, m), dtype)
        chain.process(dx, dy, m)
        got[:, o:o + m] = dy.download()
    return got


def check(tag, got_row, x_row, case, refs=None, window=None):
    e_go, e_gpu, e_orc, bound = judge(got_row, x_row, case, refs=refs, window=window)
    from f32judge import fp32_noise
    b1 = 2 * e_orc + fp32_noise(case["bq"]) + 1e-6
    print("%s e_go %.3e e_gpu %.3e e_orc %.3e bound %.3e" % (tag, e_go, e_gpu, e_orc, b1))
    assert e_go < 1e-5, (tag, "first clause", e_go)
    assert e_gpu <= min(bound, b1), (tag, "float64 clause", e_gpu, b1)


def case_of(mode, hi, hq, osc=FS4, bq=None):
    return dict(mode=int(mode), hi=hi, hq=hq, oi=osc[0], oq=osc[1], bq=bq)


def signal(rng, ch, n):
    return rng.integers(-20000, 20001, (ch, n)).astype(np.int16)


# ------------------------------------------------------------------------------------------------ 1. every channel its own bandwidth
def test_64_channels_64_bandwidths_ticks_and_one_long_call(ctx, orc):
    rng = np.random.default_rng(1)
    ch = 64
    taps = bank_taps(ch)
    assert len({t.tobytes() for t in taps}) == ch                      # 64 distinct filters: more than MSDR_MAX_TAPSETS
    x = signal(rng, ch, 12 * B)
    for step in (B, 12 * B):
        chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, taps[0], taps[0], mode=AM)
        chain.set_taps_channels_f32(0, taps)
        got = run(ctx, chain, x, step)
        info = chain.info()
        assert info["kernel"].startswith(PC), info
        assert info["flavour"] & 0x8000 and info["flavour"] & msdr.FLAVOUR_TAPS_PC, info
        for c in range(ch):
            check("bank step %d ch %d" % (step, c), got[c], x[c], case_of(AM, taps[c], taps[c]))
        chain.close()


# ------------------------------------------------------------------------------------------------ 1b. the bank the feature is for
def test_4096_channels_196_bandwidths_tick_and_long_call_cadence(ctx, orc):
    """4096 receivers on the menu's 196 bandwidths (dealt round the bank), Fs/4, AM, two-stage cascade; 4 x 128-sample ticks + one 8192-sample call,
    and the same stream as one long call.  Judged: a sample of channels -- both ends, the wrap of the menu, one in every 97 -- on the long part."""
    rng = np.random.default_rng(11)
    ch, n = 4096, 4 * B + 8192
    taps = bank_taps(ch)
    assert len({t.tobytes() for t in taps}) == 196
    bq = cascade("lp+notch")
    x = signal(rng, ch, n)
    sample = sorted(set([0, 1, 195, 196, 197, 2047, 4094, 4095] + list(range(0, ch, 97))))
    refs = {}
    for cadence in ("ticks", "long"):
        chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, taps[0], taps[0], mode=AM, biquad_coeffs=bq)
        chain.set_taps_channels_f32(0, taps)
        got = np.concatenate([run(ctx, chain, x[:, :4 * B], B), run(ctx, chain, x[:, 4 * B:])], axis=1) if cadence == "ticks" else run(ctx, chain, x)
        info = chain.info()
        assert info["kernel"].startswith(PC) and info["flavour"] & msdr.FLAVOUR_TAPS_PC and info["flavour"] & msdr.FLAVOUR_SEQ_CASCADE, info
        for c in sample:
            case = case_of(AM, taps[c], taps[c], bq=bq)
            if c not in refs:
                from f32judge import references
                refs[c] = references(x[c], case)
            check("bank4096 %s ch %d" % (cadence, c), got[c], x[c], case, refs=refs[c], window=slice(4 * B, n))
            check("bank4096 %s ch %d all" % (cadence, c), got[c], x[c], case, refs=refs[c])
        chain.close()


# ------------------------------------------------------------------------------------------------ 2. mixed bank
def test_mixed_bank_shared_sets_beside_own_taps(ctx, orc):
    rng = np.random.default_rng(2)
    ch, calls = 35, 5
    am, ssb, cw = bw_taps(2400.0), hilbert_pair(NT), hilbert_pair(NT, 700.0, 300.0)
    sets_i, sets_q = [am, ssb[0], cw[0]], [am, ssb[1], cw[1]]
    modes = np.array([(AM, LSB, USB, CW, AM)[c % 5] for c in range(ch)], np.int32)
    tapsets = np.array([(0, 1, 1, 2, 0)[c % 5] for c in range(ch)], np.int32)
    chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, sets_i, sets_q, modes=modes, tapsets=tapsets)
    own = {c: bw_taps(300.0 + 50.0 * c) for c in range(ch) if c % 5 == 0}          # the AM channels c % 5 == 0 get their own; c % 5 == 4 stay shared
    for c, t in own.items():
        chain.set_taps_channels_f32(c, t[None, :])
    n = 3 * B
    x = signal(rng, ch, calls * n)
    got = np.empty((ch, calls * n), np.float32)
    want = np.empty_like(got)
    truth = np.empty((ch, calls * n), np.float64)
    states = {c: {} for c in range(ch)}

    def tick(k):
        sl = slice(k * n, (k + 1) * n)
        got[:, sl] = run(ctx, chain, x[:, sl], B if k % 2 == 0 else None)
        assert chain.info()["kernel"].startswith(PC)
        for c in range(ch):
            ci, cq = (own[c], own[c]) if c in own else (sets_i[tapsets[c]], sets_q[tapsets[c]])
            want[c, sl] = orc.chain_f32(x[c, sl], int(modes[c]), ci, cq, FS4[0], FS4[1], state=states[c])
            truth[c, sl] = truth64(x[c, :(k + 1) * n], int(modes[c]), ci, cq, FS4[0], FS4[1], None)[sl]

    tick(0)
    am2 = bw_taps(1800.0)                                              # set_taps(tapset) changes the channels still on that tap set only
    chain.set_taps(0, am2, am2)
    sets_i[0] = sets_q[0] = am2
    tick(1)
    chain.set_taps(1, cw[0], cw[1])
    sets_i[1], sets_q[1] = cw[0], cw[1]
    tick(2)
    chain.set_mode(10, USB, 1)                                         # set_mode returns a channel to a shared set: its own taps are dropped
    modes[10], tapsets[10] = USB, 1
    del own[10]
    chain.set_mode(5, AM, 0)
    del own[5]
    tick(3)
    chain.set_taps_channels_f32(10, bw_taps(700.0)[None, :])           # and gets new ones again
    own[10] = bw_taps(700.0)
    tick(4)
    for c in range(ch):
        for k in range(calls):
            sl = slice(k * n, (k + 1) * n)
            check("mixed call %d ch %d" % (k, c), got[c], x[c], case_of(modes[c], am, am), refs=(want[c], truth[c], None), window=sl)
    chain.close()


# ------------------------------------------------------------------------------------------------ 3. general oscillator, set_osc mid-stream
def test_general_oscillator_and_set_osc_mid_stream(ctx, orc):
    rng = np.random.default_rng(3)
    ch = 12
    o1, o2 = nco128(3), nco128(5)
    modes = np.array([(AM, LSB, USB, CW)[c % 4] for c in range(ch)], np.int32)
    ssb = hilbert_pair(NT)
    ti = np.stack([bw_taps(400.0 + 300.0 * c) if modes[c] == AM else ssb[0] * np.float32(1.0 - 0.01 * c) for c in range(ch)])
    tq = np.stack([ti[c] if modes[c] == AM else ssb[1] * np.float32(1.0 - 0.01 * c) for c in range(ch)])
    n = 6 * B
    x = signal(rng, ch, 2 * n)
    chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, ti[0], ti[0], mixer=msdr.MIXER_NCO, modes=modes, osc_i=o1[0], osc_q=o1[1])
    chain.set_taps_channels_f32(0, ti, tq)
    got = np.concatenate([run(ctx, chain, x[:, :3 * B], B), run(ctx, chain, x[:, 3 * B:n])], axis=1)
    assert chain.info()["kernel"].startswith(PC)
    for c in range(ch):
        check("nco ch %d" % c, got[c], x[c, :n], case_of(modes[c], ti[c], tq[c], o1))
    chain.set_osc(o2[0], o2[1])                                        # the history keeps the table of its own time
    got2 = np.concatenate([run(ctx, chain, x[:, n:n + 3 * B], B), run(ctx, chain, x[:, n + 3 * B:])], axis=1)
    assert chain.info()["kernel"].startswith(PC)
    t = np.arange(2 * n)
    for c in range(ch):
        st = {}
        w1 = orc.chain_f32(x[c, :n], int(modes[c]), ti[c], tq[c], o1[0], o1[1], state=st)
        w2 = orc.chain_f32(x[c, n:], int(modes[c]), ti[c], tq[c], o2[0], o2[1], state=st)
        # float64: the mixer products with each sample's own table, then the FIR pair over the whole stream
        oi = np.where(t < n, o1[0].astype(np.float64)[t % 128], o2[0].astype(np.float64)[t % 128])
        oq = np.where(t < n, o1[1].astype(np.float64)[t % 128], o2[1].astype(np.float64)[t % 128])
        from scipy.signal import lfilter
        xf = x[c].astype(np.float64) / 32768.0
        ai, aq = lfilter(ti[c].astype(np.float64)[::-1], [1.0], xf * oq), lfilter(tq[c].astype(np.float64)[::-1], [1.0], xf * oi)
        tr = ai - aq if modes[c] == LSB else ai + aq if modes[c] == USB else np.sqrt(ai * ai + aq * aq)
        check("set_osc ch %d" % c, np.concatenate([got[c], got2[c]]), x[c], case_of(modes[c], ti[c], tq[c], o2),
              refs=(np.concatenate([w1, w2]), tr, None), window=slice(n, 2 * n))
    chain.close()


# ------------------------------------------------------------------------------------------------ 4. long filters, odd tap counts
@pytest.mark.parametrize("ntaps", [255, 511, 256, 512])
def test_long_tap_counts(ctx, orc, ntaps):
    rng = np.random.default_rng(40 + ntaps)
    ch, n = 6, 4096 + 77
    ssb = hilbert_pair(ntaps)
    modes = np.array([AM, USB, AM, LSB, AM, AM], np.int32)
    ti = np.stack([bw_taps(500.0 + 600.0 * c, ntaps) if modes[c] == AM else ssb[0] for c in range(ch)])
    tq = np.stack([ti[c] if modes[c] == AM else ssb[1] for c in range(ch)])
    x = signal(rng, ch, n)
    for osc in (None, nco128()):
        chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, ti[0], ti[0], modes=modes, mixer=msdr.MIXER_NCO if osc else msdr.MIXER_FS4,
                           osc_i=osc[0] if osc else None, osc_q=osc[1] if osc else None)
        chain.set_taps_channels_f32(0, ti, tq)
        got = run(ctx, chain, x)
        info = chain.info()
        assert info["kernel"].startswith(PC) and info["tile"] == 512, info         # one channel per wave
        for c in range(ch):
            check("%d taps %s ch %d" % (ntaps, "nco" if osc else "fs4", c), got[c], x[c], case_of(modes[c], ti[c], tq[c], osc or FS4))
        chain.close()


# ------------------------------------------------------------------------------------------------ 5. two-stage cascade, segmented long call
def test_two_stage_cascade_on_a_segmented_long_call(ctx, orc):
    rng = np.random.default_rng(5)
    ch, n = 3, (1 << 17) + 333
    bq = cascade("lp+notch")
    taps = np.stack([bw_taps(b) for b in (125.0, 2400.0, 5000.0)])
    x = signal(rng, ch, n + 5000)
    chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, taps[1], taps[1], mode=AM, biquad_coeffs=bq)
    warm = run(ctx, chain, x[:, :1000])                                  # the cascade runs inside the uniform kernel first ...
    assert not chain.info()["kernel"].startswith(PC)
    chain.set_taps_channels_f32(0, taps[[0]])
    chain.set_taps_channels_f32(2, taps[[2]])                            # ... and moves behind chain_f32pc_kernel with its state
    got = np.concatenate([warm, run(ctx, chain, x[:, 1000:1000 + n])], axis=1)
    info = chain.info()
    assert info["kernel"].startswith(PC) and info["time_segments"] > 1, info
    assert info["flavour"] & msdr.FLAVOUR_SEGMENTED and info["flavour"] & msdr.FLAVOUR_SEQ_CASCADE and info["flavour"] & msdr.FLAVOUR_TAPS_PC, info
    got = np.concatenate([got, run(ctx, chain, x[:, 1000 + n:])], axis=1)
    seg = -(-n // info["time_segments"])
    seg = -(-seg // info["tile"]) * info["tile"]
    wins = [("head", slice(1000, 1000 + 2048)), ("tail", slice(1000 + n - 1500, 1000 + n)), ("call", slice(1000, 1000 + n)), ("next", slice(1000 + n, n + 5000))]
    wins += [("boundary%d" % s, slice(1000 + s * seg - 512, 1000 + s * seg + 512)) for s in range(1, info["time_segments"]) if s * seg + 64 <= n][:6]
    for c in range(ch):
        case = case_of(AM, taps[c], taps[c], bq=bq)
        st = {}
        w0 = orc.chain_f32(x[c, :1000], AM, taps[1], taps[1], FS4[0], FS4[1], bq, state=st)
        w1 = orc.chain_f32(x[c, 1000:], AM, taps[c], taps[c], FS4[0], FS4[1], bq, state=st)
        # float64 with the change of filter: the demodulated stream pieced together, then the cascade over all of it
        from scipy.signal import lfilter
        d = np.concatenate([truth64(x[c], AM, taps[1], taps[1], FS4[0], FS4[1], None)[:1000], truth64(x[c], AM, taps[c], taps[c], FS4[0], FS4[1], None)[1000:]])
        for s in np.asarray(bq, np.float64):
            d = lfilter(s[:3], [1.0, -s[3], -s[4]], d)
        pre = np.concatenate([orc.chain_f32(x[c, :1000], AM, taps[1], taps[1], FS4[0], FS4[1], None, state=(s2 := {})),
                              orc.chain_f32(x[c, 1000:], AM, taps[c], taps[c], FS4[0], FS4[1], None, state=s2)])
        for name, w in wins:
            check("segmented ch %d %s" % (c, name), got[c], x[c], case, refs=(np.concatenate([w0, w1]), d, pre), window=w)
    chain.close()


# ------------------------------------------------------------------------------------------------ 5b. msdr_chain_config.time_segments
@pytest.mark.parametrize("segments", [1, 3])
def test_time_segments_of_the_configuration_are_honoured(ctx, orc, segments):
    rng = np.random.default_rng(55 + segments)
    ch, n = 2, 1 << 15
    taps = np.stack([bw_taps(700.0), bw_taps(3100.0)])
    x = signal(rng, ch, n)
    chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, taps[0], taps[0], mode=AM, time_segments=segments)
    chain.set_taps_channels_f32(0, taps)
    got = run(ctx, chain, x)
    info = chain.info()
    assert info["kernel"].startswith(PC) and info["time_segments"] == segments, info
    assert bool(info["flavour"] & msdr.FLAVOUR_SEGMENTED) == (segments > 1), info
    for c in range(ch):
        check("time_segments %d ch %d" % (segments, c), got[c], x[c], case_of(AM, taps[c], taps[c]))
    chain.close()


# ------------------------------------------------------------------------------------------------ 6. int16 audio
def test_out_i16_within_one_lsb(ctx, orc):
    rng = np.random.default_rng(6)
    ch = 16
    taps = bank_taps(ch)
    bq = cascade("lp")
    x = signal(rng, ch, 6 * B)
    for step in (B, None):
        chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, taps[0], taps[0], mode=AM, biquad_coeffs=bq, flags=msdr.CHAIN_OUT_I16)
        chain.set_taps_channels_f32(0, taps)
        got = run(ctx, chain, x, step, np.int16)
        assert chain.info()["kernel"].startswith(PC)
        for c in range(ch):
            want = orc.chain_f32(x[c], AM, taps[c], taps[c], FS4[0], FS4[1], bq)
            wi = np.clip(np.round(want.astype(np.float64) * 32768.0), -32768, 32767)
            assert np.abs(got[c].astype(np.float64) - wi).max() <= 1, (step, c)
            assert np.abs(got[c]).max() > 100
        chain.close()


# ------------------------------------------------------------------------------------------------ 7. SYNCAM under the PLL, LMS
def _post_err(got, want, pre):
    ref = max(np.sqrt((want.astype(np.float64) ** 2).sum()), np.sqrt((pre.astype(np.float64) ** 2).sum()))
    return float(np.sqrt(((got.astype(np.float64) - want) ** 2).sum()) / max(ref, 1e-300))


def test_syncam_pll_and_lms_channels_beside_plain_ones(ctx, orc):
    """The PLL and LMS rows go through the chain's auxiliary chain, which must filter with the CHANNEL's rows (every row here has a bandwidth of its
    own; the shared set is a seventh one).
    LMS rows, in two parts as tests/test_gpu_chain_post.py has them (the filter's leak control decides per sample, so its output is discontinuous in
    its input): (1) the audio in front of the filter -- a second chain with the same rows and the filter off -- through f32judge.judge, both clauses;
    (2) the chain's output against the oracle's filter applied to THAT audio: bit for bit (no cascade here), and 1e-5 of the level in front.
    The SYNCAM row: e_go < 1e-5 against the oracle's PLL.  No float64 clause can be formed for it -- the contract's float64 reference
    (f32judge.truth64) has no PLL, a feedback loop with decisions of its own, and none is written here -- so the clause is held where the row's
    arithmetic is linear: what the PLL is fed, I + Q and I - Q of the channel's own rows (the auxiliary chain's two rows for it), judged with both
    clauses on a companion chain that runs those rows as USB and LSB channels."""
    rng = np.random.default_rng(7)
    ch, n = 6, 8 * B
    taps = np.stack([bw_taps(1200.0 + 500.0 * c) for c in range(ch)])
    shared = bw_taps(600.0)
    modes = np.array([AM, SYNCAM, AM, AM, AM, SYNCAM], np.int32)
    t = np.arange(n)
    x = np.round(9000 * (1 + 0.5 * np.sin(2 * np.pi * 400 * t / 24000.0)) * np.cos(2 * np.pi * (6000.0 + 3.0) * t / 24000.0)
                 + rng.normal(0, 200, (ch, n))).astype(np.int16)
    anr = np.array([0, 0, 0, 1, 2, 1], np.int32)
    for step in (B, None):
        chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, shared, shared, modes=modes, flags=msdr.CHAIN_SYNCAM_PLL)
        chain.set_anr(anr)
        chain.set_taps_channels_f32(0, taps)
        got = run(ctx, chain, x, step)
        assert chain.info()["kernel"].startswith(PC)
        front_chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, shared, shared, modes=modes, flags=msdr.CHAIN_SYNCAM_PLL)
        front_chain.set_taps_channels_f32(0, taps)
        front = run(ctx, front_chain, x, step)                      # the audio in front of the LMS filter
        side = msdr.Chain(ctx, msdr.ARITH_F32, 2 * ch, shared, shared, modes=np.array([USB, LSB] * ch, np.int32))
        side.set_taps_channels_f32(0, np.repeat(taps, 2, axis=0))
        sides = run(ctx, side, np.repeat(x, 2, axis=0), step)       # I + Q, I - Q of every channel's own rows
        for c in range(ch):
            pll = bool(modes[c] == SYNCAM)
            tag = "post step %s ch %d mode %d anr %d" % (step, c, modes[c], anr[c])
            if pll:
                check(tag + " I+Q", sides[2 * c], x[c], case_of(USB, taps[c], taps[c]))
                check(tag + " I-Q", sides[2 * c + 1], x[c], case_of(LSB, taps[c], taps[c]))
            st, want = {}, []
            for o in range(0, n, step or n):
                want.append(orc.chain_f32(x[c, o:o + (step or n)], int(modes[c]), taps[c], taps[c], FS4[0], FS4[1], state=st, pll=pll))
            want = np.concatenate(want)                              # the oracle in front of the LMS filter (PLL included)
            if anr[c]:
                if pll:
                    e = rel_rms(front[c], want)
                    print("%s front e_go %.3e" % (tag, e))
                    assert e < 1e-5, (tag, "front", e)
                else:
                    check(tag + " front", front[c], x[c], case_of(AM, taps[c], taps[c]))
                filt = orc.anr_f32(orc.anr_new(), int(anr[c]), front[c])
                e = _post_err(got[c], filt, front[c])
                print("%s filter on the chain's own front audio %.3e" % (tag, e))
                assert np.array_equal(got[c], filt), (tag, "the filter's arithmetic is the oracle's, bit for bit")
                assert e < 1e-5, (tag, e)
                assert rel_rms(got[c], front[c]) > 1e-3, (tag, "the filter ran")
            elif pll:
                e = rel_rms(got[c], want)
                print("%s e_go %.3e" % (tag, e))
                assert e < 1e-5, (tag, e)
                assert rel_rms(got[c], orc.chain_f32(x[c], AM, taps[c], taps[c], FS4[0], FS4[1])) > 1e-2, (tag, "the PLL demodulates differently from the envelope")
            else:
                check(tag, got[c], x[c], case_of(AM, taps[c], taps[c]))
        for o in (chain, front_chain, side):
            o.close()


# ------------------------------------------------------------------------------------------------ 8. change mid-stream, reset, init_fir
@pytest.mark.parametrize("step", [B, None])
def test_change_mid_stream_and_survival(ctx, orc, step):
    rng = np.random.default_rng(8)
    ch, n = 16, 3 * B
    am = bw_taps(2400.0)
    chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, am, am, mode=AM)
    x = signal(rng, ch, 5 * n)
    cur = [am] * ch
    states = [{} for _ in range(ch)]
    hist0 = [0] * ch                      # where the stream that feeds the FIR history starts (init_fir / reset clear it)

    def ticks(k, tag):
        sl = slice(k * n, (k + 1) * n)
        got = run(ctx, chain, x[:, sl], step)
        for c in range(ch):
            want = orc.chain_f32(x[c, sl], AM, cur[c], cur[c], FS4[0], FS4[1], state=states[c])
            xs = x[c, hist0[c]:(k + 1) * n]
            tr = truth64(xs, AM, cur[c], cur[c], *_fs4_at(hist0[c]), None)[-n:]
            check("%s ch %d" % (tag, c), got[c], x[c, sl], case_of(AM, cur[c], cur[c]), refs=(want, tr, None))

    def _fs4_at(t0):                      # the mixer's position carries on over init_fir: tables rotated to the stream's own start
        return np.roll(FS4[0], -(t0 % 4)), np.roll(FS4[1], -(t0 % 4))

    ticks(0, "uniform")
    assert not chain.info()["kernel"].startswith(PC)
    t1 = bank_taps(ch)
    chain.set_taps_channels_f32(0, t1)
    cur = list(t1)
    ticks(1, "changed over the old history")
    assert chain.info()["kernel"].startswith(PC)
    t2 = np.stack([bw_taps(4000.0 - 30.0 * c) for c in range(5, 11)])
    chain.set_taps_channels_f32(5, t2)
    for c in range(5, 11):
        cur[c] = t2[c - 5]
    ticks(2, "changed again")
    chain.init_fir()                      # FIR state only; the rows stay
    for c in range(ch):
        states[c]["hist_i"][:] = 0
        states[c]["hist_q"][:] = 0
        hist0[c] = 3 * n
    ticks(3, "after init_fir")
    chain.reset()
    states = [{} for _ in range(ch)]
    x[:, 4 * n:] = x[:, :n]
    hist0 = [4 * n] * ch
    ticks(4, "after reset")
    assert chain.info()["kernel"].startswith(PC)
    chain.close()


# ------------------------------------------------------------------------------------------------ 9. identical rows = the uniform chain
def test_identical_rows_agree_with_the_oracle_as_the_uniform_chain(ctx, orc):
    rng = np.random.default_rng(9)
    ch = 8
    am = bw_taps(2400.0)
    bq = cascade("lp+notch")
    x = signal(rng, ch, 16 * B)
    uni = msdr.Chain(ctx, msdr.ARITH_F32, ch, am, am, mode=AM, biquad_coeffs=bq)
    pc = msdr.Chain(ctx, msdr.ARITH_F32, ch, am, am, mode=AM, biquad_coeffs=bq)
    pc.set_taps_channels_f32(0, np.tile(am, (ch, 1)))
    gu, gp = run(ctx, uni, x), run(ctx, pc, x)
    assert pc.info()["kernel"].startswith(PC) and not uni.info()["kernel"].startswith(PC)
    for c in range(ch):
        case = case_of(AM, am, am, bq=bq)
        check("uniform ch %d" % c, gu[c], x[c], case)
        check("identical rows ch %d" % c, gp[c], x[c], case)
    uni.close()
    pc.close()


# ------------------------------------------------------------------------------------------------ 10. a chain that never calls the setter
def test_untouched_chain_runs_what_it_ran(ctx, orc):
    rng = np.random.default_rng(10)
    ch = 8
    am = bw_taps(2400.0)
    bq = cascade("lp+notch")
    for n, kern in ((B, "chain_mfb_kernel"), (8192, "chain_mfw_kernel")):
        x = signal(rng, ch, n)
        a = msdr.Chain(ctx, msdr.ARITH_F32, ch, am, am, mode=AM, biquad_coeffs=bq)
        b = msdr.Chain(ctx, msdr.ARITH_F32, ch, am, am, mode=AM, biquad_coeffs=bq)
        touched = msdr.Chain(ctx, msdr.ARITH_F32, ch, am, am, mode=AM, biquad_coeffs=bq)
        touched.set_taps_channels_f32(0, am[None, :])
        ga, gb, _ = run(ctx, a, x), run(ctx, b, x), run(ctx, touched, x)
        ia, ib = a.info(), b.info()
        assert (ia["kernel"], ia["flavour"]) == (ib["kernel"], ib["flavour"]) and np.array_equal(ga, gb)
        assert ia["kernel"].startswith(kern) or ia["kernel"].startswith("chain_amtr_kernel"), ia       # the uniform kernels of this shape, as before
        assert not ia["flavour"] & msdr.FLAVOUR_TAPS_PC and PC not in ia["kernel"]
        assert touched.info()["kernel"].startswith(PC)
        for c in (a, b, touched):
            c.close()


# ------------------------------------------------------------------------------------------------ 11. refusals
def test_refusals(ctx):
    am = bw_taps(2400.0)
    q = msdr.Chain(ctx, msdr.ARITH_Q15, 4, np.zeros(NT, np.int16), np.zeros(NT, np.int16), mode=AM)
    with pytest.raises(msdr.MsdrError, match="F32"):
        q.set_taps_channels_f32(0, am[None, :])
    f = msdr.Chain(ctx, msdr.ARITH_F32, 4, am, am, mode=AM)
    with pytest.raises(msdr.MsdrError, match="Q15"):
        f.set_taps_channels(0, np.zeros((1, NT), np.int16))             # the Q15 entry point keeps refusing fp32 chains
    with pytest.raises(msdr.MsdrError):
        f.set_taps_channels_f32(3, np.tile(am, (2, 1)))                 # past `channels`
    with pytest.raises(msdr.MsdrError):
        f.set_taps_channels_f32(4, am[None, :])
    with pytest.raises(ValueError):
        f.set_taps_channels_f32(0, am[None, :-1])                       # wrong tap count: refused before any library call
    with pytest.raises(ValueError):
        f.set_taps_channels_f32(0, am)
    import ctypes as C
    assert ctx.lib.msdr_chain_set_taps_channels_f32(f.h, C.c_uint32(0), C.c_uint32(1), None, None) == msdr.STATUS_ARGUMENT_ERROR
    assert ctx.lib.msdr_chain_set_taps_channels_f32(f.h, C.c_uint32(0), C.c_uint32(0), None, None) == 0          # count == 0 does nothing
    assert not f.info()["kernel"].startswith(PC)
    # a graph made before the first call is refused afterwards; graph creation in per-channel mode is refused (ARGUMENT_ERROR)
    xs = [ctx.to_device(np.zeros((4, B), np.int16)) for _ in range(2)]
    ys = [ctx.array((4, B), np.float32) for _ in range(2)]
    f.process(xs[0], ys[0], B)
    f.process(xs[1], ys[1], B)
    g = f.graph(xs, ys, B)
    g.launch()
    f.set_taps_channels_f32(1, am[None, :])
    with pytest.raises(msdr.MsdrError):
        g.launch()
    with pytest.raises(msdr.MsdrError, match="not capturable"):
        f.graph(xs, ys, B)
    f.process(xs[0], ys[0], B)
    assert f.info()["kernel"].startswith(PC)
    fir = msdr.FirF32(ctx, am, 4)
    with pytest.raises(msdr.MsdrError):
        fir.set_coeffs_channels(2, np.tile(am, (3, 1)))
    with pytest.raises(ValueError):
        fir.set_coeffs_channels(0, am[None, :50])
    for o in (q, f, fir):
        o.close()


# ------------------------------------------------------------------------------------------------ 12. the arm_fir_f32 stage
@pytest.mark.parametrize("ntaps", [NT, 37, 511])
def test_fir_stage_per_channel(ctx, orc, ntaps):
    rng = np.random.default_rng(120 + ntaps)
    ch, n = 9, 12 * B
    rows = bank_taps(ch, ntaps)
    x = rng.standard_normal((ch, n)).astype(np.float32)
    for step in (B, None):
        fir = msdr.FirF32(ctx, rows[0], ch)
        got = np.empty_like(x)
        first = 2 * B                                                    # the uniform kernel first: the change-over keeps the history
        for o, m in ((0, first),) + tuple((o, step or n - first) for o in range(first, n, step or n - first)):
            if o == first:
                fir.set_coeffs_channels(1, rows[1:])
            dx, dy = ctx.to_device(np.ascontiguousarray(x[:, o:o + m])), ctx.array((ch, m), np.float32)
            fir.process(dx, dy, m)
            got[:, o:o + m] = dy.download()
        for c in range(ch):
            want = np.concatenate([orc.fir_f32_blocks(rows[0], x[c], B)[:first], orc.fir_f32_blocks(rows[c], x[c], B)[first:]])
            e = rel_rms(got[c], want)
            print("fir %d taps step %s ch %d %.3e" % (ntaps, step, c, e))
            assert e <= 1e-6, (ntaps, step, c, e)
        fir.set_coeffs(rows[2])                                          # keeps writing all channels
        dx, dy = ctx.to_device(np.ascontiguousarray(x[:, :B])), ctx.array((ch, B), np.float32)
        fir.reset()
        fir.process(dx, dy, B)
        y = dy.download()
        for c in range(ch):
            assert rel_rms(y[c], orc.fir_f32_blocks(rows[2], x[c, :B], B)) <= 1e-6, c
        fir.close()


def test_per_channel_rows_take_a_chain_off_the_folded_kernel(ctx, orc):
    """Per-channel coefficients come before the oscillator fold in msdr_chain_process: a chain on chain_fold_kernel<4> (Fs/4, MSDR_CHAIN_NO_MFMA)
    runs chain_f32pc_kernel from the first call after the rows arrive -- the same samples as from a chain that never folded (no cascade: the
    raw history is all the state there is)."""
    rng = np.random.default_rng(77)
    ch = 5
    taps = bank_taps(ch)
    x = signal(rng, ch, 3 * B + 40)
    outs = []
    for flags in (msdr.CHAIN_NO_MFMA, 0):
        chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, taps[0], taps[0], mode=LSB, flags=flags)
        run(ctx, chain, x[:, :B])
        if flags:
            assert chain.info()["kernel"] == "chain_fold_kernel<4>", chain.info()
        chain.set_taps_channels_f32(0, taps)
        outs.append(run(ctx, chain, x[:, B:]))
        assert chain.info()["kernel"].startswith(PC) and chain.info()["flavour"] & msdr.FLAVOUR_TAPS_PC, chain.info()
        chain.close()
    assert np.array_equal(outs[0], outs[1])
