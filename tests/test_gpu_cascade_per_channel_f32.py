"""Per-receiver fp32 cascade coefficients: msdr_biquad_df1_f32_set_coeffs_channels / msdr_chain_set_biquad_coeffs_channels give single channels
cascade coefficients of their own; biquad_df1_seq_pc_kernel runs arm_biquad_cascade_df1_f32 in CMSIS order with every lane its own rows.

The stage is held to the project's gate for it, 2e-6 relative RMS against the oracle's arm_biquad_cascade_df1_f32 with that channel's
coefficients and carried pState, and to bit-identity with the uniform CMSIS-order kernel where all rows are equal.  The chain is judged
channel by channel through f32judge.judge at level 1 -- e_go < 1e-5 and e_gpu <= 2 e_orc + fp32_noise + 1e-6, no case excused
(tests/test_cascade_pc_cases.py holds the cases to that)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import cascade_pc_cases as cc
import orclib
from f32judge import fp32_noise, judge, references
from f32pc_cases import B, FS4, NT, bw_taps
from gpuhelp import ctx, msdr, rel_rms  # noqa: F401

pytestmark = pytest.mark.gpu
PCK = " + biquad_df1_seq_pc_kernel"
AM, LSB, USB = orclib.AM, orclib.LSB, orclib.USB
GATE = 2e-6


def stage_run(ctx, inst, x, offset_view=False):
    """one call of the stage on x [ch, n]; offset_view: on an array view one float off 16-byte alignment"""
    ch, n = x.shape
    if not offset_view:
        dx, dy = ctx.to_device(np.ascontiguousarray(x)), ctx.array((ch, n), np.float32)
        inst.process(dx, dy, n)
        return dy.download()
    flat = np.zeros(ch * n + 4, np.float32)
    flat[1:1 + ch * n] = x.reshape(-1)
    d = ctx.to_device(flat)
    inst.process(d.offset(4), d.offset(4), n)                           # in place, unaligned
    return d.download()[1:1 + ch * n].reshape(ch, n)


def chain_run(ctx, chain, x, step=None):
    ch, n = x.shape
    got = np.empty((ch, n), np.float32)
    step = step or n
    for o in range(0, n, step):
        m = min(step, n - o)
        dx, dy = ctx.to_device(np.ascontiguousarray(x[:, o:o + m])), ctx.array((ch, m), np.float32)
        chain.process(dx, dy, m)
        got[:, o:o + m] = dy.download()
    return got


def check(tag, got_row, x_row, case, refs=None, window=None):
    e_go, e_gpu, e_orc, bound = judge(got_row, x_row, case, refs=refs, window=window)
    b1 = 2 * e_orc + fp32_noise(case["bq"]) + 1e-6
    print("%s e_go %.3e e_gpu %.3e e_orc %.3e bound %.3e" % (tag, e_go, e_gpu, e_orc, b1))
    assert e_go < 1e-5, (tag, "first clause", e_go)
    assert e_gpu <= min(bound, b1), (tag, "float64 clause", e_gpu, b1)


def flavours(info, *bits):
    return all(info["flavour"] & b for b in bits)


# ------------------------------------------------------------------------------------------------ 1. bit-identity with the uniform kernel
def test_stage_equal_rows_are_bit_identical_to_the_uniform_cmsis_order_kernel(ctx):
    ch, n = 65, 3 * 128 + 5
    hp = cc.highpass_pair()
    a, b = msdr.BiquadDf1F32(ctx, hp, ch), msdr.BiquadDf1F32(ctx, hp, ch)
    b.set_coeffs_channels(0, np.tile(hp[None], (ch, 1, 1)))
    for k in range(3):
        x = cc.audio(100 + k, ch, n)
        ya, yb = stage_run(ctx, a, x), stage_run(ctx, b, x)
        assert np.array_equal(ya, yb), k
        assert np.abs(ya).max() > 1e-3
    for c in (0, 63, 64):
        assert np.array_equal(a.cmsis_state(c, 2), b.cmsis_state(c, 2)), c
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 2. every channel its own filter
@pytest.mark.parametrize("stages", [1, 2, 3, 4])
@pytest.mark.parametrize("ch", [1, 63, 64, 130])
def test_stage_every_channel_its_own_filter(ctx, ch, stages):
    rows = cc.stage_rows(ch, stages, offset=stages)
    for n in (128, 131):
        inst = msdr.BiquadDf1F32(ctx, rows[0], ch)
        inst.set_coeffs_channels(0, rows)
        orcs = [cc.Df1(rows[c]) for c in range(ch)]
        for k in range(4):                                              # three calls, and one more on an unaligned view
            x = cc.audio(1000 * stages + 10 * n + k, ch, n)
            got = stage_run(ctx, inst, x, offset_view=(k == 3))
            for c in range(ch):
                want = orcs[c].run(x[c])
                e = rel_rms(got[c], want)
                assert e <= GATE, (ch, stages, n, k, c, e)
            for c in sorted({0, ch // 2, ch - 1}):
                st = inst.cmsis_state(c, stages)
                assert st[0] == x[c, -1] and st[1] == x[c, -2], (c, "stage 0 keeps the last two inputs")
                assert st[4 * stages - 2] == got[c, -1] and st[4 * stages - 1] == got[c, -2], (c, "the last stage keeps the last two outputs")
        inst.close()


# ------------------------------------------------------------------------------------------------ 3. a coefficient change keeps the state
def test_stage_coefficient_change_keeps_state(ctx):
    ch, n, stages = 5, 256, 2
    rows = cc.stage_rows(ch, stages)
    new = cc.stage_rows(ch, stages, offset=3)
    x1, x2 = cc.audio(31, ch, n), cc.audio(32, ch, n)
    inst, plain = msdr.BiquadDf1F32(ctx, rows[0], ch), msdr.BiquadDf1F32(ctx, rows[0], ch)
    inst.set_coeffs_channels(0, rows)
    plain.set_coeffs_channels(0, rows)
    orcs = [cc.Df1(rows[c]) for c in range(ch)]
    stage_run(ctx, inst, x1)
    stage_run(ctx, plain, x1)
    for c in range(ch):
        orcs[c].run(x1[c])
    for c in (1, 3):
        inst.set_coeffs_channels(c, new[c][None])
        orcs[c].set_coeffs(new[c])                                      # the same pCoeffs swap over the oracle's kept pState
        assert not np.array_equal(new[c], rows[c])
    got, ref = stage_run(ctx, inst, x2), stage_run(ctx, plain, x2)
    for c in range(ch):
        want = orcs[c].run(x2[c])
        for tag, w in (("call", slice(0, n)), ("first 64", slice(0, 64))):
            e = rel_rms(got[c, w], want[w])
            print("change ch %d %s %.3e" % (c, tag, e))
            assert e <= GATE, (c, tag, e)
    for c in (0, 2, 4):
        assert np.array_equal(got[c], ref[c]), c
    for c in (1, 3):
        assert rel_rms(got[c], ref[c]) > 1e-3, c
    inst.close()
    plain.close()


# ------------------------------------------------------------------------------------------------ 4. conversion at the first call
def test_stage_first_call_converts_a_block_parallel_instance_with_its_state(ctx):
    ch, n = 6, 2048
    uniform = cc.lp_notch3k()
    assert msdr.biquad_cascade_info(uniform)[2] == 0                    # block-parallel
    rows = cc.bank_rows(ch)
    inst = msdr.BiquadDf1F32(ctx, uniform, ch)
    orcs = [cc.Df1(uniform) for _ in range(ch)]
    x1, x2 = cc.audio(41, ch, n), cc.audio(42, ch, n)
    g1 = stage_run(ctx, inst, x1)
    inst.set_coeffs_channels(0, rows)
    g2 = stage_run(ctx, inst, x2)
    for c in range(ch):
        w1 = orcs[c].run(x1[c])
        orcs[c].set_coeffs(rows[c])
        w2 = orcs[c].run(x2[c])
        for tag, g, w in (("before", g1[c], w1), ("after", g2[c], w2), ("first 64 after", g2[c, :64], w2[:64]), ("both", np.concatenate([g1[c], g2[c]]), np.concatenate([w1, w2]))):
            e = rel_rms(g, w)
            print("conversion ch %d %s %.3e" % (c, tag, e))
            assert e <= GATE, (c, tag, e)
    inst.close()


# ------------------------------------------------------------------------------------------------ 5. time segments
SEG_CH, SEG_N = 3, 65536


def _seg_rows():
    lp = cc.lowpass()
    return np.stack([np.stack([lp, cc.notch(3000.0, 15.0)]), np.stack([lp, cc.notch(1500.0, 2.0)]), np.stack([lp, cc.PASS])])


def _seg_plan():
    """(segments, segment length) by the sizing of msdr_biquad_df1_f32_process, from the LARGEST pole radius over the rows: warm-up =
    log(1e-10) / log(r) + 64 stages (a multiple of 4), segments of at least 8 warm-ups (and 1024 samples), at most 65536 / channels of them,
    segment starts on multiples of 4 samples.  The largest radius is the notch Q 15 at 3 kHz's, 0.9767: warm-up 1108, 65536 // 8864 = 7
    segments of 9364 samples (the last one 9352)."""
    radius = max(max(np.abs(np.roots([1.0, -s[3], -s[4]])).max() for s in r.astype(np.float64) if s[3] or s[4]) for r in _seg_rows())
    warm = (int(np.ceil(np.log(1e-10) / np.log(radius))) + 64 * 2 + 3) & ~3
    nseg = max(1, min(-(-65536 // SEG_CH), SEG_N // max(8 * warm, 1024)))
    seg_len = (-(-SEG_N // nseg) + 3) & ~3
    return -(-SEG_N // seg_len), seg_len


def _seg_check(got, x, tag):
    rows = _seg_rows()
    nseg, seg_len = _seg_plan()
    for c in range(SEG_CH):
        want = cc.Df1(rows[c]).run(x[c])
        wins = [("call", slice(0, SEG_N))] + [("boundary %d" % s, slice(s * seg_len - 256, s * seg_len + 256)) for s in range(1, nseg)]
        for name, w in wins:
            e = rel_rms(got[c, w], want[w])
            print("%s ch %d %s %.3e" % (tag, c, name, e))
            assert e <= GATE, (tag, c, name, e)


def test_stage_long_block_of_few_channels_runs_in_time_segments(ctx):
    rows = _seg_rows()
    assert _seg_plan() == (7, 9364), _seg_plan()                        # the call IS split, and the windows below sit on its boundaries
    x = cc.audio(51, SEG_CH, SEG_N)
    inst = msdr.BiquadDf1F32(ctx, rows[2], SEG_CH)
    inst.set_coeffs_channels(0, rows)
    got = stage_run(ctx, inst, x)
    _seg_check(got, x, "segmented")
    tail = cc.audio(52, SEG_CH, 512)                                    # the state the last segment left: the stream carries on
    g2 = stage_run(ctx, inst, tail)
    for c in range(SEG_CH):
        o = cc.Df1(rows[c])
        o.run(x[c])
        assert rel_rms(g2[c], o.run(tail[c])) <= GATE, c
    inst.close()


def test_stage_long_block_with_segments_switched_off_in_a_child_process():
    """MSDR_BIQUAD_SEQ_NO_SEGMENTS is read when an instance is created: a fresh process, the same data, the same bound."""
    env = dict(os.environ, MSDR_BIQUAD_SEQ_NO_SEGMENTS="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--no-segments-child"], env=env, capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0 and "no-segments child OK" in r.stdout


def _no_segments_child():
    c = msdr.Context(0)
    rows = _seg_rows()
    x = cc.audio(51, SEG_CH, SEG_N)
    inst = msdr.BiquadDf1F32(c, rows[2], SEG_CH)
    inst.set_coeffs_channels(0, rows)
    _seg_check(stage_run(c, inst, x), x, "one piece")
    inst.close()
    c.close()
    print("no-segments child OK")


# ------------------------------------------------------------------------------------------------ 6. refusals of the stage
def test_stage_refusals_change_nothing(ctx):
    ch, n = 4, 200
    rows = cc.stage_rows(ch, 2)
    inst, orcs = msdr.BiquadDf1F32(ctx, rows[0], ch), [cc.Df1(rows[0]) for _ in range(ch)]
    f = ctx.lib.msdr_biquad_df1_f32_set_coeffs_channels
    arr = np.ascontiguousarray(rows.reshape(ch, 10))
    p = arr.ctypes.data_as(C.c_void_p)
    assert f(inst.h, C.c_uint32(3), C.c_uint32(2), p) == msdr.STATUS_ARGUMENT_ERROR            # past `channels`
    assert f(inst.h, C.c_uint32(4), C.c_uint32(1), p) == msdr.STATUS_ARGUMENT_ERROR
    assert f(inst.h, C.c_uint32(0), C.c_uint32(1), None) == msdr.STATUS_ARGUMENT_ERROR         # NULL array
    assert f(inst.h, C.c_uint32(9), C.c_uint32(0), None) == 0                                  # count == 0 does nothing
    with pytest.raises(msdr.MsdrError):
        inst.set_coeffs_channels(2, rows)
    with pytest.raises(ValueError):
        inst.set_coeffs_channels(0, rows[:, :1])
    empty = msdr.BiquadDf1F32(ctx, np.zeros(0, np.float32), ch)                                # numStages == 0
    assert f(empty.h, C.c_uint32(0), C.c_uint32(1), p) == msdr.STATUS_ARGUMENT_ERROR
    x = cc.audio(61, ch, n)
    got, thru = stage_run(ctx, inst, x), stage_run(ctx, empty, x)
    assert np.array_equal(thru, x)                                                              # the empty cascade still passes its input
    for c in range(ch):
        assert rel_rms(got[c], orcs[c].run(x[c])) <= GATE, c                                    # the unchanged filter
    inst.close()
    empty.close()


# ------------------------------------------------------------------------------------------------ 7. the bank
def test_chain_bank_of_64_receivers_each_its_own_notch(ctx, orc):
    ch, taps = cc.BANK_CH, bw_taps(2400.0)
    rows, x = cc.bank_rows(ch), cc.bank_input()
    refs = {}
    for step in (B, cc.BANK_N):
        chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, taps, taps, mode=AM, biquad_coeffs=rows[0])
        chain.set_biquad_coeffs_channels(0, rows)
        got = chain_run(ctx, chain, x, step)
        info = chain.info()
        assert info["kernel"].endswith(PCK), info
        assert flavours(info, msdr.FLAVOUR_CASCADE_PC, msdr.FLAVOUR_SEQ_CASCADE) and not info["flavour"] & msdr.FLAVOUR_TAPS_PC, info
        for c in range(ch):
            case = cc.case_of(AM, taps, taps, rows[c])
            if c not in refs:
                refs[c] = references(x[c], case)
            check("bank step %d ch %d" % (step, c), got[c], x[c], case, refs=refs[c])
        chain.close()


# ------------------------------------------------------------------------------------------------ 8. together with per-channel taps
def test_chain_per_channel_taps_and_per_channel_cascade_in_both_orders(ctx, orc):
    ch, x, taps, rows = cc.BOTH_CH, cc.both_input(), cc.both_taps(), cc.bank_rows(cc.BOTH_CH, 1)
    refs = {}
    for order in ("taps first", "cascade first"):
        chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, taps[0], taps[0], mode=AM, biquad_coeffs=rows[0])
        if order == "taps first":
            chain.set_taps_channels_f32(0, taps)
            chain.set_biquad_coeffs_channels(0, rows)
        else:
            chain.set_biquad_coeffs_channels(0, rows)
            chain.set_taps_channels_f32(0, taps)
        got = chain_run(ctx, chain, x, 2 * B)
        info = chain.info()
        assert info["kernel"].startswith("chain_f32pc_kernel") and info["kernel"].endswith(PCK), info
        assert flavours(info, msdr.FLAVOUR_TAPS_PC, msdr.FLAVOUR_CASCADE_PC, msdr.FLAVOUR_SEQ_CASCADE), info
        for c in range(ch):
            case = cc.case_of(AM, taps[c], taps[c], rows[c])
            if c not in refs:
                refs[c] = references(x[c], case)
            check("%s ch %d" % (order, c), got[c], x[c], case, refs=refs[c])
        chain.close()
    # equal rows = the uniform cascade behind chain_f32pc_kernel, bit for bit
    same = cc.lp_notch3k()
    a = msdr.Chain(ctx, msdr.ARITH_F32, ch, taps[0], taps[0], mode=AM, biquad_coeffs=same)
    b = msdr.Chain(ctx, msdr.ARITH_F32, ch, taps[0], taps[0], mode=AM, biquad_coeffs=same)
    a.set_taps_channels_f32(0, taps)
    b.set_taps_channels_f32(0, taps)
    b.set_biquad_coeffs_channels(0, np.tile(same[None], (ch, 1, 1)))
    ga, gb = chain_run(ctx, a, x, 2 * B), chain_run(ctx, b, x, 2 * B)
    assert a.info()["kernel"].endswith(" + biquad_df1_seq_kernel") and b.info()["kernel"].endswith(PCK)
    assert np.array_equal(ga, gb)
    check("uniform cascade ch 0", ga[0], x[0], cc.case_of(AM, taps[0], taps[0], same))
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 9. the first call moves the cascade mid-stream
def test_chain_first_call_moves_the_cascade_out_of_the_matrix_core_kernel_mid_stream(ctx, orc):
    m, x, n = cc.move_setup(), cc.move_input(), cc.MOVE_CALL
    chain = msdr.Chain(ctx, msdr.ARITH_F32, 2, m["sets_i"], m["sets_q"], modes=m["modes"], tapsets=m["tapsets"], biquad_coeffs=m["uniform"])
    got = [chain_run(ctx, chain, x[:, k * n:(k + 1) * n]) for k in range(2)]
    info = chain.info()
    assert "biquad_df1" not in info["kernel"] and not info["flavour"] & msdr.FLAVOUR_SEQ_CASCADE, info          # the cascade ran inside the kernel
    chain.set_biquad_coeffs_channels(0, m["rows"])
    got += [chain_run(ctx, chain, x[:, k * n:(k + 1) * n]) for k in range(2, 4)]
    info = chain.info()
    assert info["kernel"].endswith(PCK) and flavours(info, msdr.FLAVOUR_CASCADE_PC, msdr.FLAVOUR_SEQ_CASCADE), info
    got = np.concatenate(got, axis=1)
    for c in range(2):
        ts = m["tapsets"][c]
        want, truth = cc.stream_refs(x[c], m["modes"][c], m["sets_i"][ts], m["sets_q"][ts], [(0, m["uniform"]), (2 * n, m["rows"][c])])
        after = cc.case_of(m["modes"][c], m["sets_i"][ts], m["sets_q"][ts], m["rows"][c])
        stream = dict(after, bq=max((m["uniform"], m["rows"][c]), key=fp32_noise))          # (the larger noise figure of the stream's two cascades)
        check("moved ch %d stream" % c, got[c], x[c], stream, refs=(want, truth, None))
        check("moved ch %d after" % c, got[c], x[c], after, refs=(want, truth, None), window=slice(2 * n, 4 * n))
    chain.close()


# ------------------------------------------------------------------------------------------------ 10. survival and interplay
def test_chain_rows_survive_every_live_update_and_reset(ctx, orc):
    ch, n = 6, 2 * B
    am, am2 = bw_taps(2400.0), bw_taps(1800.0)
    ssb = cc.hilbert_pair(NT)
    rows = cc.bank_rows(ch)
    k128 = np.arange(128)
    o1 = ((np.round(32767 * np.sin(2 * np.pi * 3 * k128 / 128)).astype(np.int16) / 32768.0).astype(np.float32),
          (np.round(32767 * np.cos(2 * np.pi * 3 * k128 / 128)).astype(np.int16) / 32768.0).astype(np.float32))
    o2 = (np.roll(o1[0], 17).copy(), np.roll(o1[1], 17).copy())
    x = cc.signal(101, ch, 7 * n)
    chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, [am, ssb[0]], [am, ssb[1]], mixer=msdr.MIXER_NCO, osc_i=o1[0], osc_q=o1[1], mode=AM, biquad_coeffs=rows[0])
    chain.set_biquad_coeffs_channels(0, rows)
    cur = dict(taps=[(am, am)] * ch, mode=[AM] * ch, osc=o1, rows=[r for r in rows])
    states = [{} for _ in range(ch)]

    def tick(k, tag):
        sl = slice(k * n, (k + 1) * n)
        got = chain_run(ctx, chain, x[:, sl], B)
        info = chain.info()
        assert info["kernel"].endswith(PCK) and flavours(info, msdr.FLAVOUR_CASCADE_PC, msdr.FLAVOUR_SEQ_CASCADE), (tag, info)
        for c in range(ch):
            want = orc.chain_f32(x[c, sl], cur["mode"][c], cur["taps"][c][0], cur["taps"][c][1], cur["osc"][0], cur["osc"][1], cur["rows"][c], state=states[c])
            e = rel_rms(got[c], want)
            print("%s ch %d e_go %.3e" % (tag, c, e))
            assert e < 1e-5, (tag, c, e)
        return got

    tick(0, "per-channel rows")
    chain.set_taps(0, am2, am2)
    cur["taps"] = [(am2, am2)] * ch
    tick(1, "after set_taps")
    chain.set_mode(2, USB, 1)
    cur["mode"][2], cur["taps"][2] = USB, ssb
    tick(2, "after set_mode")
    chain.set_osc(o2[0], o2[1])
    # (the oracle mixes every sample with the table of its own time, as the chain does: its FIR history holds mixed samples)
    cur["osc"] = o2
    tick(3, "after set_osc")
    chain.init_fir()
    for c in range(ch):
        states[c]["hist_i"][:] = 0
        states[c]["hist_q"][:] = 0
    tick(4, "after init_fir")
    chain.reset()                                                       # clears state only: the rows still answer
    states = [{} for _ in range(ch)]
    got5 = tick(5, "after reset")
    assert max(rel_rms(got5[0], got5[c]) for c in range(1, ch)) > 1e-3  # the channels do run different filters
    chain.set_biquad_coeffs(rows[3])                                    # writes every channel's row; the chain stays in per-channel mode
    cur["rows"] = [rows[3]] * ch
    cur["mode"][2], cur["taps"][2] = AM, (am2, am2)
    chain.set_mode(2, AM, 0)
    chain.reset()
    states = [{} for _ in range(ch)]
    x[:, 6 * n:] = x[0, 6 * n:]                                         # one input for all: equal rows give equal channels
    got6 = tick(6, "after set_biquad_coeffs")
    for c in range(1, ch):
        assert np.array_equal(got6[0], got6[c]), c
    chain.close()


# ------------------------------------------------------------------------------------------------ 11. refusals of the chain
def test_chain_refusals(ctx):
    am = bw_taps(2400.0)
    rows = cc.bank_rows(4)
    q = msdr.Chain(ctx, msdr.ARITH_Q15, 4, np.zeros(NT, np.int16), np.zeros(NT, np.int16), mode=AM)
    q.stages = 2                                                        # (past the binding's own shape check: the library refuses)
    with pytest.raises(msdr.MsdrError, match="F32") as e:
        q.set_biquad_coeffs_channels(0, rows)
    assert e.value.status == msdr.STATUS_ARGUMENT_ERROR
    none = msdr.Chain(ctx, msdr.ARITH_F32, 4, am, am, mode=AM)
    none.stages = 2
    with pytest.raises(msdr.MsdrError, match="without a biquad cascade") as e:
        none.set_biquad_coeffs_channels(0, rows)
    assert e.value.status == msdr.STATUS_ARGUMENT_ERROR
    pll = msdr.Chain(ctx, msdr.ARITH_F32, 4, am, am, mode=AM, biquad_coeffs=rows[0], flags=msdr.CHAIN_SYNCAM_PLL)
    with pytest.raises(msdr.MsdrError, match="SYNCAM_PLL") as e:
        pll.set_biquad_coeffs_channels(0, rows)
    assert e.value.status == msdr.STATUS_ARGUMENT_ERROR
    # an LMS channel on: the call is refused and the output is what it was
    x = cc.signal(111, 4, 2 * B)
    lms, twin = (msdr.Chain(ctx, msdr.ARITH_F32, 4, am, am, mode=AM, biquad_coeffs=rows[0]) for _ in range(2))
    for c in (lms, twin):
        c.set_anr(np.array([0, 1, 0, 0], np.int32))
    with pytest.raises(msdr.MsdrError, match="LMS") as e:
        lms.set_biquad_coeffs_channels(0, rows)
    assert e.value.status == msdr.STATUS_ARGUMENT_ERROR
    assert np.array_equal(chain_run(ctx, lms, x, B), chain_run(ctx, twin, x, B))
    assert PCK not in lms.info()["kernel"]
    # per-channel cascade first: LMS channels are refused, switching them all off is not
    f = msdr.Chain(ctx, msdr.ARITH_F32, 4, am, am, mode=AM, biquad_coeffs=rows[0])
    f.set_biquad_coeffs_channels(0, rows)
    with pytest.raises(msdr.MsdrError, match="LMS") as e:
        f.set_anr(np.array([0, 0, 2, 0], np.int32))
    assert e.value.status == msdr.STATUS_ARGUMENT_ERROR
    with pytest.raises(msdr.MsdrError):
        f.set_anr(None, 1)
    f.set_anr(None, 0)
    with pytest.raises(msdr.MsdrError):
        f.set_biquad_coeffs_channels(3, rows[:2])                       # past `channels`
    with pytest.raises(ValueError):
        f.set_biquad_coeffs_channels(0, rows[:, :1])
    g = ctx.lib.msdr_chain_set_biquad_coeffs_channels
    assert g(f.h, C.c_uint32(0), C.c_uint32(1), None) == msdr.STATUS_ARGUMENT_ERROR
    assert g(f.h, C.c_uint32(0), C.c_uint32(0), None) == 0
    xs = [ctx.to_device(np.zeros((4, B), np.int16)) for _ in range(2)]
    ys = [ctx.array((4, B), np.float32) for _ in range(2)]
    with pytest.raises(msdr.MsdrError) as e:                            # a cascade behind the kernel: no graph
        f.graph(xs, ys, B)
    assert e.value.status == msdr.STATUS_ARGUMENT_ERROR
    f.process(xs[0], ys[0], B)
    assert f.info()["kernel"].endswith(PCK)
    for o in (q, none, pll, lms, twin, f):
        o.close()


if __name__ == "__main__" and "--no-segments-child" in sys.argv:
    _no_segments_child()
