"""Per-receiver phase-accumulator oscillator for the fp32 chain: msdr_chain_set_nco_channels tunes each receiver to ANY frequency;
chain_f32pcn_kernel computes channel ch's oscillator (the Q15 values / 32768, exact in fp32) from its own {phase, step}; the cascade runs
behind it in CMSIS order.

Every channel is judged on its own through f32judge.judge, exactly as tests/test_gpu_osc_per_channel_f32.py judges: e_go < 1e-5 against
orclib.Oracle.chain_f32 and e_gpu <= 2 e_orc + fp32_noise + 1e-6 against float64 on every row -- no new tolerance.  Both references get the
oscillator VALUES of each sample's own time as a table as long as the signal (the model of tests/test_gpu_nco_per_channel.py)."""
import ctypes as C

import numpy as np
import pytest

import orclib
from f32pc_cases import B, NT, bw_taps, cascade, hilbert_pair
from gpuhelp import ctx, msdr  # noqa: F401
from test_gpu_nco_per_channel import Bank, M32, off_grid_steps, u32
from test_gpu_osc_per_channel_f32 import check, refs_of, rows, run, signal

pytestmark = pytest.mark.gpu
PCN = "chain_f32pcn_kernel"
AM, LSB, USB = orclib.AM, orclib.LSB, orclib.USB


def f32(v):
    return (v.astype(np.float64) / 32768.0).astype(np.float32)


def any_table():
    oi, oq = rows(1, 128, seed=3)
    return dict(osc_i=oi[0], osc_q=oq[0])


def bank_of(kind, ch):
    """AM: 102 taps, a bandwidth per channel; LSB: the 100-tap Hilbert pair, a gain per channel"""
    if kind == "am":
        t = np.stack([bw_taps(700.0 + 600.0 * c) for c in range(ch)])
        return AM, t, t
    hi, hq = hilbert_pair(100)
    g = (1.0 - 0.02 * np.arange(ch)).astype(np.float32)
    return LSB, hi[None, :] * g[:, None], hq[None, :] * g[:, None]


# ------------------------------------------------------------------------------------------------ 6. ticks, a segmented call, int16 output
@pytest.mark.parametrize("kind", ["am", "lsb"])
@pytest.mark.parametrize("key", [None, "lp+notch"])
def test_ticks_and_a_segmented_call(ctx, orc, kind, key):
    rng = np.random.default_rng(1060 + (kind == "am") + 2 * (key is None))
    ch, n = 6, 8 * B
    bq = cascade(key)
    mode, ti, tq = bank_of(kind, ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    x = signal(rng, ch, n)
    si, sq = Bank(steps, phases).advance(n)
    si, sq = f32(si), f32(sq)
    refs = [refs_of(orc, x[c], mode, ti[c], tq[c], si[c], sq[c], bq) for c in range(ch)]
    want_flav = msdr.FLAVOUR_NCO_PC | msdr.FLAVOUR_TAPS_PC | (msdr.FLAVOUR_SEQ_CASCADE if key else 0)
    for step, segs in ((B, 0), (n, 2)):
        chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, ti[0], tq[0], mixer=msdr.MIXER_NCO, mode=mode, biquad_coeffs=bq, time_segments=segs, **any_table())
        chain.set_nco_channels(0, u32(steps), u32(phases))
        chain.set_taps_channels_f32(0, ti, tq)
        bank = Bank(steps, phases)
        got = np.empty((ch, n), np.float32)
        for o in range(0, n, step):
            got[:, o:o + step] = run(ctx, chain, x[:, o:o + step])
            bank.advance(step)
            bank.check(chain, (step, o))
        info = chain.info()
        assert info["kernel"].startswith(PCN), info
        assert info["flavour"] & want_flav == want_flav and info["flavour"] & 0x80000, info
        assert not info["flavour"] & (msdr.FLAVOUR_OSC_PC | msdr.FLAVOUR_BLOCK), info
        assert bool(info["flavour"] & msdr.FLAVOUR_SEQ_CASCADE) == bool(key), info
        assert bool(info["flavour"] & msdr.FLAVOUR_SEGMENTED) == (segs == 2) and info["time_segments"] == max(segs, 1), info
        if step == B:          # f32pcn_lds_bytes: 4 waves x 4 channels of chain_f32pc_kernel's area (no row per channel) + ONE 4 096-byte sine table
            assert info["lds_bytes"] == 16 * 4 * (2 * 256 + 2 * 128) + 4096, info
        for c in range(ch):
            check("%s %s step %d ch %d" % (kind, key, step, c), got[c], x[c], refs[c], bq)
        chain.close()


def test_int16_output_is_within_one_lsb(ctx, orc):
    rng = np.random.default_rng(1066)
    ch, n = 6, 4 * B
    bq = cascade("lp")
    taps = np.stack([bw_taps(1500.0 + 300.0 * c) for c in range(ch)])
    # every receiver near the carrier the input has (6000 Hz), off the table grid
    steps = np.array([msdr.nco_step(6000.0 + 3.3 * c - 7.0) for c in range(ch)], np.uint64)
    phases = rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    t = np.arange(n)
    x = np.round(12000 * (1 + 0.5 * np.sin(2 * np.pi * 400 * t / 24000.0)) * np.cos(2 * np.pi * 6000.0 * t / 24000.0) + rng.normal(0, 200, (ch, n))).astype(np.int16)
    si, sq = Bank(steps, phases).advance(n)
    chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, taps[0], taps[0], mixer=msdr.MIXER_NCO, mode=AM, biquad_coeffs=bq, flags=msdr.CHAIN_OUT_I16, **any_table())
    chain.set_taps_channels_f32(0, taps)
    chain.set_nco_channels(0, u32(steps), u32(phases))
    got = run(ctx, chain, x, B, np.int16)
    assert chain.info()["kernel"].startswith(PCN)
    for c in range(ch):
        want = orc.chain_f32(x[c], AM, taps[c], taps[c], f32(si[c]), f32(sq[c]), bq)
        wi = np.clip(np.round(want.astype(np.float64) * 32768.0), -32768, 32767)
        assert np.abs(got[c].astype(np.float64) - wi).max() <= 1, c
        assert np.abs(got[c]).max() > 100
    chain.close()


# ------------------------------------------------------------------------------------------------ 2. bit-identity with the table path
def test_on_the_128_grid_the_chain_equals_the_table_chain_bit_for_bit(ctx):
    """steps k_c * 2^25 with the low-pass + notch cascade: both paths run the same functions on the same values"""
    rng = np.random.default_rng(1062)
    ch, n = 7, 4 * B
    bq = cascade("lp+notch")
    ti = np.stack([bw_taps(500.0 + 450.0 * c) for c in range(ch)])
    k = np.array([0, 1, 5, 32, 64, 127, 77], np.uint64)
    j = np.array([0, 0, 17, 1, 127, 5, 90], np.uint64)
    ph = (((j[:, None] + k[:, None] * np.arange(128, dtype=np.uint64)[None, :]) << np.uint64(25)) & M32).astype(np.uint32)
    s, c = msdr.nco_q15(ph)
    oi, oq = f32(s.reshape(ch, 128)), f32(c.reshape(ch, 128))
    x = signal(rng, ch, n)
    a, b = (msdr.Chain(ctx, msdr.ARITH_F32, ch, ti[0], ti[0], mixer=msdr.MIXER_NCO, mode=AM, osc_i=oi[0], osc_q=oq[0], biquad_coeffs=bq) for _ in range(2))
    for o in (a, b):
        o.set_taps_channels_f32(0, ti)
    a.set_nco_channels(0, u32(k << np.uint64(25)), u32(j << np.uint64(25)))
    b.set_osc_channels(0, oi, oq)
    for lo, hi in ((0, B), (B, 3 * B), (3 * B, 4 * B)):
        ga, gb = run(ctx, a, x[:, lo:hi]), run(ctx, b, x[:, lo:hi])
        assert np.array_equal(ga.view(np.uint32), gb.view(np.uint32)), (lo, hi)
        assert np.abs(ga).max() > 1e-3
    assert a.info()["kernel"].startswith(PCN) and b.info()["kernel"].startswith("chain_f32pco_kernel")
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ 7. refusals leave the chain untouched
def test_refusals_leave_the_chain_untouched(ctx, orc):
    rng = np.random.default_rng(1067)
    ch = 6
    am = bw_taps(2400.0)
    bq = cascade("lp+notch")
    x = signal(rng, ch, 2 * B)
    steps, phases = u32(off_grid_steps(rng, ch)), u32(rng.integers(0, 1 << 32, ch, dtype=np.uint64))
    lib = ctx.lib
    ERR = msdr.STATUS_ARGUMENT_ERROR

    def call(chain, first, count, a, b=None):
        return lib.msdr_chain_set_nco_channels(chain.h, C.c_uint32(first), C.c_uint32(count),
                                               None if a is None else a.ctypes.data_as(C.c_void_p), None if b is None else b.ctypes.data_as(C.c_void_p))

    def table_chain(**kw):
        return msdr.Chain(ctx, msdr.ARITH_F32, ch, am, am, mixer=msdr.MIXER_NCO, mode=AM, biquad_coeffs=bq, **any_table(), **kw)

    def same(a, b, tag):
        ga, gb = run(ctx, a, x, B), run(ctx, b, x, B)
        assert np.array_equal(ga.view(np.uint32), gb.view(np.uint32)), tag
        assert a.info() == b.info(), tag

    fs4, fs4_control = (msdr.Chain(ctx, msdr.ARITH_F32, ch, am, am, mode=AM, biquad_coeffs=bq) for _ in range(2))
    assert call(fs4, 0, ch, steps) == ERR                                             # the Fs/4 mixer has no oscillator to tune
    same(fs4, fs4_control, "fs4")
    a, a_control = table_chain(), table_chain()
    assert call(a, 0, ch, None, phases) == ERR                                        # a NULL step array
    assert call(a, 4, 3, steps) == ERR                                                # 4 .. 6 of 6
    assert call(a, 1, ch - 1, steps) == ERR                                           # a partial first call
    assert call(a, 0, 0, None) == 0                                                   # count == 0 does nothing
    same(a, a_control, "table chain")
    assert PCN not in a.info()["kernel"]
    assert call(a, 0, ch, steps, phases) == ERR                                       # samples have been processed: the history is not clear
    same(a, a_control, "first call over a used history")
    pll, pll_control = table_chain(flags=msdr.CHAIN_SYNCAM_PLL), table_chain(flags=msdr.CHAIN_SYNCAM_PLL)
    assert call(pll, 0, ch, steps, phases) == ERR                                     # PLL channels run through the auxiliary chain
    same(pll, pll_control, "pll")
    lms, lms_control = table_chain(), table_chain()
    for o in (lms, lms_control):
        o.set_anr(np.array([0, 1, 0, 0, 2, 0], np.int32))
    assert call(lms, 0, ch, steps, phases) == ERR                                     # ... and so do LMS channels
    same(lms, lms_control, "lms")
    osc, osc_control = table_chain(), table_chain()
    oi, oq = rows(ch, 128)
    for o in (osc, osc_control):
        o.set_osc_channels(0, oi, oq)
    assert call(osc, 0, ch, steps, phases) == ERR                                     # per-channel oscillator tables exclude the phase accumulator
    same(osc, osc_control, "table rows")
    n1, n1_control = table_chain(), table_chain()
    for o in (n1, n1_control):
        o.set_nco_channels(0, steps, phases)
    for f in (lambda: n1.set_osc(oi[0], oq[0]), lambda: n1.set_osc_channels(0, oi, oq), lambda: n1.set_anr(np.array([0, 1, 0, 0, 0, 0], np.int32)),
              lambda: n1.set_anr(None, 1), lambda: n1.graph([ctx.array((ch, B), np.int16) for _ in range(2)], [ctx.array((ch, B), np.float32) for _ in range(2)], B)):
        with pytest.raises(msdr.MsdrError) as e:
            f()
        assert e.value.status == ERR
    n1.set_anr(None, 0)                                                               # no channel on: accepted
    n1.set_block_kernel(True)                                                         # accepted: such calls run the unfused launches
    same(n1, n1_control, "nco chain")
    info = n1.info()
    assert info["kernel"].startswith(PCN) and not info["flavour"] & msdr.FLAVOUR_BLOCK, info
    for o in (fs4, fs4_control, a, a_control, pll, pll_control, lms, lms_control, osc, osc_control, n1, n1_control):
        o.close()
