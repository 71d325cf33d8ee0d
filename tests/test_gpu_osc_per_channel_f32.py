"""Per-receiver oscillator tables for the fp32 chain: msdr_chain_set_osc_channels gives single channels table rows of their own;
chain_f32pco_kernel mixes channel ch with row ch, the cascade runs behind it in CMSIS order.

Every channel is judged on its own through f32judge.judge, exactly as tests/test_gpu_taps_per_channel_f32.py judges: e_go < 1e-5 against
orclib.Oracle.chain_f32 with that channel's own tables, and e_gpu <= 2 e_orc + fp32_noise + 1e-6 against float64 on every row.  Both
references get the table VALUES that were in force when each sample arrived (the oracle's FIR history holds mixed samples): a table as
long as the call, the position counted from the call's start."""
import ctypes as C

import numpy as np
import pytest
from scipy.signal import lfilter

import orclib
from f32judge import fp32_noise, judge
from f32pc_cases import B, NT, bw_taps, cascade, hilbert_pair
from gpuhelp import ctx, msdr  # noqa: F401

pytestmark = pytest.mark.gpu
PCO = "chain_f32pco_kernel"
AM, LSB, USB, CW, SYNCAM = orclib.AM, orclib.LSB, orclib.USB, orclib.CW, orclib.SYNCAM


def rows(ch, L, seed=0):
    """(osc_i, osc_q) [ch, L] float32: a different bin and a different start phase per channel (Q15 table values / 32768)"""
    k = (1 + seed + 3 * np.arange(ch)) % L
    ph = 0.37 * (1 + seed) + 0.61 * np.arange(ch)
    a = 2 * np.pi * k[:, None] * np.arange(L)[None, :] / L + ph[:, None]
    return ((np.round(32767 * np.sin(a)).astype(np.int16) / 32768.0).astype(np.float32),
            (np.round(32767 * np.cos(a)).astype(np.int16) / 32768.0).astype(np.float32))


def at(tab, pos, n):
    return tab[:, (pos + np.arange(n)) % tab.shape[1]]


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


def refs_of(orc, x, mode, hi, hq, si, sq, bq):
    """(oracle, float64, oracle without the cascade) of one channel's whole stream from zero state; si / sq: the table values per SAMPLE"""
    want = orc.chain_f32(x, int(mode), hi, hq, si, sq, bq)
    pre = orc.chain_f32(x, int(mode), hi, hq, si, sq, None)
    xf = x.astype(np.float64) / 32768.0
    ai = lfilter(hi.astype(np.float64)[::-1], [1.0], xf * sq.astype(np.float64))
    aq = lfilter(hq.astype(np.float64)[::-1], [1.0], xf * si.astype(np.float64))
    d = ai - aq if mode == LSB else ai + aq if mode == USB else np.sqrt(ai * ai + aq * aq)
    if bq is not None:
        for s in np.asarray(bq, np.float64):
            d = lfilter(s[:3], [1.0, -s[3], -s[4]], d)
    return want, d, pre


def check(tag, got_row, x_row, refs, bq, window=None):
    case = dict(bq=bq)
    e_go, e_gpu, e_orc, bound = judge(got_row, x_row, case, refs=refs, window=window)
    b1 = 2 * e_orc + fp32_noise(bq) + 1e-6
    print("%s e_go %.3e e_gpu %.3e e_orc %.3e bound %.3e" % (tag, e_go, e_gpu, e_orc, b1))
    assert e_go < 1e-5, (tag, "first clause", e_go)
    assert e_gpu <= min(bound, b1), (tag, "float64 clause", e_gpu, b1)


def mixed_bank(ch, nt=NT):
    modes = np.array([(AM, LSB, USB, CW)[c % 4] for c in range(ch)], np.int32)
    ssb, cw = hilbert_pair(nt), hilbert_pair(nt, 700.0, 300.0)
    ti = np.stack([bw_taps(500.0 + 350.0 * c, nt) if modes[c] == AM else (cw if modes[c] == CW else ssb)[0] for c in range(ch)])
    tq = np.stack([ti[c] if modes[c] == AM else (cw if modes[c] == CW else ssb)[1] for c in range(ch)])
    return modes, ti, tq


def signal(rng, ch, n):
    return rng.integers(-20000, 20001, (ch, n)).astype(np.int16)


FLAV = msdr.FLAVOUR_TAPS_PC | msdr.FLAVOUR_OSC_PC | msdr.FLAVOUR_SEQ_CASCADE


# ------------------------------------------------------------------------------------------------ 1. ticks and one long call
@pytest.mark.parametrize("L", [128, 24])
def test_ticks_and_one_long_call(ctx, orc, L):
    rng = np.random.default_rng(100 + L)
    ch, n = 10, 6 * B
    bq = cascade("lp+notch")
    modes, ti, tq = mixed_bank(ch)
    oi, oq = rows(ch, L)
    x = signal(rng, ch, n)
    si, sq = at(oi, 0, n), at(oq, 0, n)
    refs = [refs_of(orc, x[c], modes[c], ti[c], tq[c], si[c], sq[c], bq) for c in range(ch)]
    for step, tile in ((B, 128), (2 * B, 256), (n, 512)):
        chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, ti[0], tq[0], mixer=msdr.MIXER_NCO, modes=modes, osc_i=oi[0], osc_q=oq[0], biquad_coeffs=bq)
        chain.set_taps_channels_f32(0, ti, tq)
        chain.set_osc_channels(0, oi, oq)
        got = run(ctx, chain, x, step)
        info = chain.info()
        assert info["kernel"].startswith(PCO) and info["tile"] == tile, info
        assert info["flavour"] & FLAV == FLAV and info["flavour"] & 0x20000, info
        assert info["kernel"].endswith("biquad_df1_seq_kernel"), info
        for c in range(ch):
            check("L %d step %d ch %d" % (L, step, c), got[c], x[c], refs[c], bq)
        chain.close()


# ------------------------------------------------------------------------------------------------ 2. live changes inside one history length
def test_live_changes_inside_one_history_length(ctx, orc):
    rng = np.random.default_rng(2)
    ch, nt, T, L = 10, 256, 32, 128
    ticks = 24
    bq = cascade("lp+notch")
    modes, ti, tq = mixed_bank(ch, nt)
    cur_i, cur_q = rows(ch, L)
    chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, ti[0], tq[0], mixer=msdr.MIXER_NCO, modes=modes, osc_i=cur_i[0], osc_q=cur_q[0], biquad_coeffs=bq)
    chain.set_osc_channels(0, cur_i, cur_q)                            # (no per-channel taps yet: the table is filled from the shared set ...)
    chain.set_taps_channels_f32(0, ti, tq)                             # (... and the two calls combine in this order too)
    x = signal(rng, ch, ticks * T)
    got = np.empty((ch, ticks * T), np.float32)
    si, sq = np.empty_like(got), np.empty_like(got)
    for k in range(ticks):
        sl = slice(k * T, (k + 1) * T)
        got[:, sl] = run(ctx, chain, x[:, sl])
        assert chain.info()["kernel"].startswith(PCO)
        si[:, sl], sq[:, sl] = at(cur_i, k * T, T), at(cur_q, k * T, T)
        if k in (2, 4, 5):
            ni, nq = rows(4, L, seed=10 + k)
            if k == 4:
                chain.set_osc_channels(3, *rows(4, L, seed=77))       # two calls in a row: the first one's rows never mix a sample
            chain.set_osc_channels(3, ni, nq)
            cur_i, cur_q = cur_i.copy(), cur_q.copy()
            cur_i[3:7], cur_q[3:7] = ni, nq
        if k == 8:
            one = rows(1, L, seed=5)
            chain.set_osc(one[0][0], one[1][0])
            cur_i, cur_q = np.tile(one[0], (ch, 1)), np.tile(one[1], (ch, 1))
    for c in range(ch):
        refs = refs_of(orc, x[c], modes[c], ti[c], tq[c], si[c], sq[c], bq)
        check("live ch %d" % c, got[c], x[c], refs, bq)
        for lo, hi in ((2 * T, 9 * T), (9 * T, 18 * T)):               # the ticks right behind the changes, one history length each
            check("live ch %d [%d, %d)" % (c, lo, hi), got[c], x[c], refs, bq, window=slice(lo, hi))
    chain.close()


# ------------------------------------------------------------------------------------------------ 3. the other per-channel setters, both orders
@pytest.mark.parametrize("order", ["osc first", "osc last"])
def test_combination_with_per_channel_taps_and_cascades(ctx, orc, order):
    rng = np.random.default_rng(3)
    ch, L, n = 7, 128, 4 * B
    bq = cascade("lp+notch")
    s = np.asarray(bq, np.float32)
    bqs = np.stack([np.stack([s[0], s[1] * np.float32([1.0, 1.0 - 0.002 * c, 1.0, 1.0 - 0.002 * c, 1.0])]) for c in range(ch)])   # a notch of its own per channel
    modes, ti, tq = mixed_bank(ch)
    oi, oq = rows(ch, L, seed=2)
    x = signal(rng, ch, n)
    chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, ti[0], tq[0], mixer=msdr.MIXER_NCO, modes=modes, osc_i=oi[0], osc_q=oq[0], biquad_coeffs=bq)
    if order == "osc first":
        chain.set_osc_channels(0, oi, oq)
    chain.set_biquad_coeffs_channels(0, bqs)
    chain.set_taps_channels_f32(0, ti, tq)
    if order == "osc last":
        chain.set_osc_channels(0, oi, oq)
    got = np.concatenate([run(ctx, chain, x[:, :2 * B], B), run(ctx, chain, x[:, 2 * B:])], axis=1)
    info = chain.info()
    assert info["kernel"].startswith(PCO) and info["kernel"].endswith("biquad_df1_seq_pc_kernel"), info
    assert info["flavour"] & (FLAV | msdr.FLAVOUR_CASCADE_PC) == FLAV | msdr.FLAVOUR_CASCADE_PC, info
    si, sq = at(oi, 0, n), at(oq, 0, n)
    for c in range(ch):
        check("%s ch %d" % (order, c), got[c], x[c], refs_of(orc, x[c], modes[c], ti[c], tq[c], si[c], sq[c], bqs[c]), bqs[c])
    chain.close()


# ------------------------------------------------------------------------------------------------ 4. refusals leave the chain untouched
def test_refusals_leave_the_chain_untouched(ctx, orc):
    rng = np.random.default_rng(4)
    ch, L = 6, 128
    am = bw_taps(2400.0)
    bq = cascade("lp+notch")
    oi, oq = rows(ch, L)
    x = signal(rng, ch, 2 * B)
    lib = ctx.lib

    def call(chain, first, count, a, b):
        return lib.msdr_chain_set_osc_channels(chain.h, C.c_uint32(first), C.c_uint32(count), None if a is None else a.ctypes.data_as(C.c_void_p),
                                               None if b is None else b.ctypes.data_as(C.c_void_p))

    def nco(**kw):
        return msdr.Chain(ctx, msdr.ARITH_F32, ch, am, am, mixer=msdr.MIXER_NCO, mode=AM, osc_i=oi[0], osc_q=oq[0], biquad_coeffs=bq, **kw)

    fs4, fs4_control = (msdr.Chain(ctx, msdr.ARITH_F32, ch, am, am, mode=AM, biquad_coeffs=bq) for _ in range(2))
    assert call(fs4, 0, ch, oi, oq) == msdr.STATUS_ARGUMENT_ERROR                     # the Fs/4 mixer has no tables
    a, a_control = nco(), nco()
    assert call(a, 0, ch, None, oq) == msdr.STATUS_ARGUMENT_ERROR                     # a NULL array, either one
    assert call(a, 0, ch, oi, None) == msdr.STATUS_ARGUMENT_ERROR
    assert call(a, 4, 3, oi, oq) == msdr.STATUS_ARGUMENT_ERROR                        # 4 .. 6 of 6
    assert call(a, 0, 0, None, None) == 0                                             # count == 0 does nothing
    bad = oi.copy()
    bad[2, 17] = np.inf
    assert call(a, 0, ch, bad, oq) == msdr.STATUS_ARGUMENT_ERROR                      # an entry that is not finite
    bad[2, 17] = np.nan
    assert call(a, 0, ch, oi, bad) == msdr.STATUS_ARGUMENT_ERROR
    with pytest.raises(ValueError):
        a.set_osc_channels(0, oi[:, :100], oq[:, :100])
    pll, pll_control = nco(flags=msdr.CHAIN_SYNCAM_PLL), nco(flags=msdr.CHAIN_SYNCAM_PLL)
    with pytest.raises(msdr.MsdrError, match="MSDR_CHAIN_SYNCAM_PLL") as e:           # PLL channels run through the auxiliary chain
        pll.set_osc_channels(0, oi, oq)
    assert e.value.status == msdr.STATUS_ARGUMENT_ERROR
    lms, lms_control = nco(), nco()
    anr = np.array([0, 1, 0, 0, 2, 0], np.int32)
    lms.set_anr(anr)
    lms_control.set_anr(anr)
    with pytest.raises(msdr.MsdrError, match="LMS") as e:
        lms.set_osc_channels(0, oi, oq)
    assert e.value.status == msdr.STATUS_ARGUMENT_ERROR
    first = {}
    for p, q in ((fs4, fs4_control), (a, a_control), (pll, pll_control), (lms, lms_control)):
        first[p], gq = run(ctx, p, x, B), run(ctx, q, x, B)
        assert np.array_equal(first[p], gq)
        assert p.info() == q.info() and PCO not in p.info()["kernel"] and not p.info()["flavour"] & msdr.FLAVOUR_OSC_PC
    # in per-channel-oscillator mode: no LMS channel can be switched on (all off is accepted), no graph
    a.set_osc_channels(0, oi, oq)
    with pytest.raises(msdr.MsdrError, match="LMS") as e:
        a.set_anr(anr)
    assert e.value.status == msdr.STATUS_ARGUMENT_ERROR
    with pytest.raises(msdr.MsdrError):
        a.set_anr(None, 1)
    a.set_anr(np.zeros(ch, np.int32))
    xs = [ctx.to_device(np.zeros((ch, B), np.int16)) for _ in range(2)]
    ys = [ctx.array((ch, B), np.float32) for _ in range(2)]
    with pytest.raises(msdr.MsdrError, match="not capturable"):
        a.graph(xs, ys, B)
    x2 = signal(rng, ch, 2 * B)
    got = run(ctx, a, x2, B)
    assert a.info()["kernel"].startswith(PCO)
    xx = np.concatenate([x, x2], axis=1)
    si = np.concatenate([at(np.tile(oi[:1], (ch, 1)), 0, 2 * B), at(oi, 2 * B, 2 * B)], axis=1)
    sq = np.concatenate([at(np.tile(oq[:1], (ch, 1)), 0, 2 * B), at(oq, 2 * B, 2 * B)], axis=1)
    for c in range(ch):                                               # the stream went on: the shared table first, then every channel its row
        check("after the refusals ch %d" % c, np.concatenate([first[a][c], got[c]]), xx[c], refs_of(orc, xx[c], AM, am, am, si[c], sq[c], bq), bq,
              window=slice(2 * B, 4 * B))
    for o in (fs4, fs4_control, a, a_control, pll, pll_control, lms, lms_control):
        o.close()


# ------------------------------------------------------------------------------------------------ 5. int16 audio
def test_out_i16_within_one_lsb(ctx, orc):
    rng = np.random.default_rng(6)
    ch, L, n = 10, 24, 6 * B
    bq = cascade("lp")
    taps = np.stack([bw_taps(1500.0 + 300.0 * c) for c in range(ch)])
    k = np.arange(L)
    # every receiver on the carrier the input has: 6 of 24 entries per cycle = 6000 Hz, its own phase
    oi = np.stack([(np.round(32767 * np.sin(2 * np.pi * 6 * k / L + 0.5 * c)).astype(np.int16) / 32768.0).astype(np.float32) for c in range(ch)])
    oq = np.stack([(np.round(32767 * np.cos(2 * np.pi * 6 * k / L + 0.5 * c)).astype(np.int16) / 32768.0).astype(np.float32) for c in range(ch)])
    t = np.arange(n)
    x = np.round(12000 * (1 + 0.5 * np.sin(2 * np.pi * 400 * t / 24000.0)) * np.cos(2 * np.pi * 6000.0 * t / 24000.0) + rng.normal(0, 200, (ch, n))).astype(np.int16)
    si, sq = at(oi, 0, n), at(oq, 0, n)
    for step in (B, None):
        chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, taps[0], taps[0], mixer=msdr.MIXER_NCO, mode=AM, osc_i=oi[0], osc_q=oq[0], biquad_coeffs=bq, flags=msdr.CHAIN_OUT_I16)
        chain.set_taps_channels_f32(0, taps)
        chain.set_osc_channels(0, oi, oq)
        got = run(ctx, chain, x, step, np.int16)
        assert chain.info()["kernel"].startswith(PCO)
        for c in range(ch):
            want = orc.chain_f32(x[c], AM, taps[c], taps[c], si[c], sq[c], bq)
            wi = np.clip(np.round(want.astype(np.float64) * 32768.0), -32768, 32767)
            assert np.abs(got[c].astype(np.float64) - wi).max() <= 1, (step, c)
            assert np.abs(got[c]).max() > 100
        chain.close()


# ------------------------------------------------------------------------------------------------ 6. equal rows = the shared table, bit for bit
@pytest.mark.parametrize("n", [128, 256, 1003])
def test_rows_that_equal_the_shared_table_give_the_taps_chain_bit_for_bit(ctx, n):
    """chain_f32pco_kernel and chain_f32pc_kernel run the same staging, FIR, demodulator and store functions and differ in the mixer policy
    alone (the row in LDS / the table in global memory): with every row equal to the shared table the audio is the same bits.  Two calls, so
    that the second starts from a history and a non-zero table position."""
    rng = np.random.default_rng(60 + n)
    ch, nt, L = 7, 30, 24
    modes, ti, tq = mixed_bank(ch, nt)
    oi, oq = rows(1, L, seed=4)
    x = signal(rng, ch, 2 * n)
    got = {}
    for kind in ("taps", "rows"):
        chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, ti[0], tq[0], mixer=msdr.MIXER_NCO, modes=modes, osc_i=oi[0], osc_q=oq[0])
        chain.set_taps_channels_f32(0, ti, tq)
        if kind == "rows":
            chain.set_osc_channels(0, np.tile(oi, (ch, 1)), np.tile(oq, (ch, 1)))
        got[kind] = run(ctx, chain, x, n)
        assert chain.info()["kernel"].startswith(PCO if kind == "rows" else "chain_f32pc_kernel"), chain.info()
        chain.close()
    assert np.abs(got["taps"]).max() > 1e-3
    assert np.array_equal(got["taps"].view(np.uint32), got["rows"].view(np.uint32)), np.flatnonzero((got["taps"] != got["rows"]).any(axis=0))[:16]
