"""The per-receiver spectrum display of the down-converter bank (F32).  The expected bins are float64 numpy.fft.fft / 64 of
tests/spectrum_model.py's tail over the DEVICE's own pairs, read back from a caller's d_iq (tests/test_gpu_iq_per_channel_f32.py holds those
to the oracle): ||dev - ref||_2 / ||ref||_2 <= 1e-5 per non-zero row, |p - p_ref| <= 2e-5 max_k p_ref per row -- the stage's bounds
(tests/test_gpu_cfft64.py).  A chain without a d_iq must give bit for bit the spectra of the chain with one, and the audio of a chain with no
spectrum.  Buffers carry a sentinel before every call and a guard row, as in the Q15 file, whose helpers these are."""
import ctypes

import numpy as np
import pytest

import orclib

import spectrum_model as M
from gpuhelp import ctx, msdr  # noqa: F401
from test_gpu_decim_per_channel_f32 import nco_chain
from test_gpu_iq_per_channel import bits
from test_gpu_nco_per_channel import off_grid_steps, u32
from test_gpu_nco_per_channel_f32 import any_table
from test_gpu_osc_per_channel_f32 import mixed_bank, signal
from test_gpu_spectrum_per_channel import B, WINDOWS, Display, call, with_tap

pytestmark = pytest.mark.gpu
ARG, LEN = msdr.STATUS_ARGUMENT_ERROR, msdr.STATUS_LENGTH_ERROR
F = np.float32
SPEC = msdr.FLAVOUR_SPECTRUM


def judged(disp, window, tag):
    """the drawn spectrum against float64 of `window` [ch, 64, 2] -> (bins, power) as read"""
    got_b, got_p = disp.read()
    assert got_b is not None or got_p is not None, (tag, "no spectrum was drawn")
    for c, w in enumerate(window):
        ref = M.cfft64_f64(w)
        p_ref = M.display(ref.real ** 2 + ref.imag ** 2)
        if not np.abs(ref).max() > 0:
            assert (got_b is None or not got_b[c].any()) and (got_p is None or not got_p[c].any()), (tag, c)
            continue
        if got_b is not None:
            dev = got_b[c].astype(np.float64)
            ratio = float(np.sqrt(((dev[:, 0] - ref.real) ** 2 + (dev[:, 1] - ref.imag) ** 2).sum()) / np.sqrt((np.abs(ref) ** 2).sum()))
            assert ratio <= 1e-5, (tag, c, ratio)
        if got_p is not None:
            err = float(np.abs(got_p[c].astype(np.float64) - p_ref).max() / p_ref.max())
            assert err <= 2e-5, (tag, c, err)
    return got_b, got_p


def fbank(ctx, ch, seed, D=1, **kw):
    rng = np.random.default_rng(seed)
    modes, ti, tq = mixed_bank(ch)
    chain = nco_chain(ctx, ch, ti, tq, off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64), modes=modes, **kw)
    if D > 1:
        chain.set_decimation(D)
    return chain, rng


# ------------------------------------------------------------------------------------------------ 1. the window
@pytest.mark.parametrize("ch", [1, 5, 17])
@pytest.mark.parametrize("case", sorted(WINDOWS))
def test_the_window_is_the_most_recent_64_pairs(ctx, case, ch):
    D, calls = WINDOWS[case]
    alone, tapped, plain = (fbank(ctx, ch, 9100 + ch + 100 * D, D)[0] for _ in range(3))
    rng = np.random.default_rng(9100 + ch)
    d_alone, d_tapped = Display(ctx, alone, ch, dtype=F), Display(ctx, tapped, ch, dtype=F)
    buf = with_tap(ctx, tapped, ch, max(calls) // D, F)
    tail = M.Tail(ch, F)
    for k, m in enumerate(calls):
        x = signal(rng, ch, m)
        d_alone.arm(); d_tapped.arm()
        a_tapped, a_alone, a_plain = (call(ctx, c, x, D, dtype=F) for c in (tapped, alone, plain))
        window = tail.push(buf.download()[:, :m // D])
        if case == "b" and k < 3:
            assert not window[:, :64 - 16 * (k + 1)].any() and window[:, -16:].any()
        got = judged(d_tapped, window, (case, k))
        same = d_alone.read()
        assert np.array_equal(bits(got[0]), bits(same[0])) and np.array_equal(bits(got[1]), bits(same[1])), (case, k)          # with and without a d_iq
        assert np.array_equal(bits(a_alone), bits(a_plain)) and np.array_equal(bits(a_tapped), bits(a_plain)), (case, k)
        assert alone.spectrum()[2:] == (1, k + 1)
    fa, fp = alone.info()["flavour"], plain.info()["flavour"]
    assert fa == fp | SPEC and not fp & SPEC and not fa & msdr.FLAVOUR_IQ_OUT and alone.info()["kernel"] == plain.info()["kernel"]
    alone.set_spectrum(None, None)          # the flavour bit exactly while on
    call(ctx, alone, signal(rng, ch, calls[0]), D, dtype=F)
    assert alone.info()["flavour"] == fp
    for c in (alone, tapped, plain):
        c.close()


# ------------------------------------------------------------------------------------------------ 2. cadence and state
def test_cadence_state_and_a_failed_call(ctx):
    ch, D = 5, 8
    chain, rng = fbank(ctx, ch, 9200, D)
    buf = with_tap(ctx, chain, ch, 16, F)
    disp, tail, model = Display(ctx, chain, ch, 3, dtype=F), M.Tail(ch, F), M.Tick(3)

    def tick(expect_draw, tag):
        disp.arm()
        call(ctx, chain, signal(rng, ch, B), D, dtype=F)
        window = tail.push(buf.download()[:, :16])
        assert model.tick() == expect_draw, tag
        if expect_draw:
            judged(disp, window, tag)
        else:
            assert disp.idle(), tag
        assert chain.spectrum()[3] == model.drawn
        return window

    for k in range(8):
        tick(k in (0, 3, 6), k)
    assert chain.spectrum()[3] == 3
    disp.arm()
    with pytest.raises(msdr.MsdrError) as e:          # counter 2: a LENGTH_ERROR call moves nothing
        chain.process(ctx.to_device(np.zeros((ch, 100), np.int16)), ctx.array((ch, 12), F), 100)
    assert e.value.status == LEN and disp.idle() and chain.spectrum()[3] == 3
    tick(False, "behind the failed call")
    chain.init_fir()          # keeps tail and counter
    assert tick(True, "across init_fir")[:, :48].any()
    chain.reset()          # clears both: the next call draws zeros ++ its own pairs
    tail.clear(); model.reset()
    assert not tick(True, "behind reset")[:, :48].any()
    chain.set_spectrum(None, None)
    chain.set_spectrum(disp.d_bins, disp.d_pow, 3)          # off -> on: tail, counter and count start over
    tail.clear(); model.reset(); model.drawn = 0
    assert not tick(True, "off -> on")[:, :48].any() and chain.spectrum()[3] == 1
    chain.close()


# ------------------------------------------------------------------------------------------------ 3. combinations
def twin_run(ctx, make, calls=4, D=8, m=B, audio_of=lambda k: True, xshape=None, pll=()):
    on, off = make(), make()
    ch = on.channels
    has_tap = on.iq_out()[0] is not None
    buf = with_tap(ctx, off, ch, m // D, F) if not has_tap else off._iq_out
    disp, tail = Display(ctx, on, ch, 1, dtype=F), M.Tail(ch, F)
    rng = np.random.default_rng(9300)
    meters = [c._meter for c in (on, off) if c.meter() is not None]
    for k in range(calls):
        x = rng.integers(-20000, 20001, xshape(ch, m) if xshape else (ch, m)).astype(np.int16)
        disp.arm()
        a_on, a_off = call(ctx, on, x, D, audio_of(k), F), call(ctx, off, x, D, audio_of(k), F)
        if audio_of(k):
            assert np.array_equal(bits(a_on), bits(a_off)), k
        if meters:
            assert np.array_equal(meters[0].download(), meters[1].download()) and meters[0].download().any(), k
        for c in pll:
            assert np.array_equal(on.pll_state(c).view(np.uint32), off.pll_state(c).view(np.uint32)) and on.pll_state(c).any(), (k, c)
        judged(disp, tail.push(buf.download()[:, :m // D]), k)
    flav = on.info()["flavour"], off.info()["flavour"]
    on.close(); off.close()
    return flav


def test_with_the_meter(ctx):
    def make():
        chain, _ = fbank(ctx, 5, 9310, 8)
        chain.set_meter(ctx.to_device(np.zeros(5, np.float64)))
        return chain
    on, off = twin_run(ctx, make)
    assert on & SPEC and not off & SPEC and on & msdr.FLAVOUR_METER and on == (off & ~msdr.FLAVOUR_IQ_OUT) | SPEC


def test_with_gain_the_spectrum_sees_the_gained_pairs(ctx):
    """the pairs the spectrum is judged against are the gained ones a d_iq receives; the meter keeps reading the ungained level"""
    def make():
        chain, _ = fbank(ctx, 5, 9315, 8)
        chain.set_meter(ctx.to_device(np.zeros(5, np.float64)))
        chain.set_gain(True)
        chain.set_gain_channels(2, np.array([4.0], np.float32))
        return chain
    on, off = twin_run(ctx, make)
    assert on & SPEC and not off & SPEC and on & msdr.FLAVOUR_GAIN and on & msdr.FLAVOUR_METER


def test_on_complex_input(ctx):
    def make():
        chain, _ = fbank(ctx, 5, 9320, 8)
        chain.set_complex_input(True, 0)
        return chain
    on, _ = twin_run(ctx, make, xshape=lambda ch, m: (ch, m, 2))
    assert on & SPEC and on & msdr.FLAVOUR_COMPLEX_IN


def test_on_a_shared_antenna_row(ctx):
    def make():
        chain, _ = fbank(ctx, 5, 9325, 8)
        chain.set_input_rows(np.zeros(5, np.int64), 1)
        return chain
    on, _ = twin_run(ctx, make, xshape=lambda ch, m: (1, m))
    assert on & SPEC and on & msdr.FLAVOUR_SHARED_IF


def test_beside_the_banks_pll(ctx):
    """MSDR_CHAIN_SYNCAM_PLL, set_bank_post, receiver 1 on SYNCAM, D = 8: bank_pll_f32_kernel and bank_cfft64_f32_kernel read the same pairs --
    the chain's own per-call buffer on the chain with the spectrum, the caller's d_iq on the one without.  Audio and PLL state bit-equal, the
    spectrum judged against the second chain's pairs, both flavour bits on the first"""
    def make():
        modes, ti, tq = mixed_bank(5)
        modes[1] = orclib.SYNCAM
        ti[1], tq[1] = ti[0], ti[0]          # (receiver 0's AM low-pass on both paths)
        rng = np.random.default_rng(9327)
        chain = msdr.Chain(ctx, msdr.ARITH_F32, 5, ti[0], tq[0], mixer=msdr.MIXER_NCO, modes=modes, flags=msdr.CHAIN_SYNCAM_PLL, **any_table())
        chain.set_bank_post(True)
        chain.set_nco_channels(0, u32(off_grid_steps(rng, 5)), u32(rng.integers(0, 1 << 32, 5, dtype=np.uint64)))
        chain.set_taps_channels_f32(0, ti, tq)
        chain.set_decimation(8)
        return chain
    on, off = twin_run(ctx, make, pll=(1,))
    both = SPEC | msdr.FLAVOUR_BANK_POST
    assert on & both == both and off & both == msdr.FLAVOUR_BANK_POST and not on & msdr.FLAVOUR_IQ_OUT and off & msdr.FLAVOUR_IQ_OUT


def test_iq_only_calls_feed_the_window(ctx):
    def make():
        chain, _ = fbank(ctx, 5, 9330, 8)
        with_tap(ctx, chain, 5, 16, F)
        return chain
    twin_run(ctx, make, calls=6, audio_of=lambda k: k % 2 == 1)


def test_with_the_block_kernel_switch_on(ctx):
    def make():
        chain, _ = fbank(ctx, 5, 9340, 1)
        chain.set_block_kernel(1)
        return chain
    on, off = twin_run(ctx, make, D=1)
    assert not on & msdr.FLAVOUR_BLOCK and not off & msdr.FLAVOUR_BLOCK


def test_refusals_change_nothing(ctx):
    ch = 5
    modes, ti, tq = mixed_bank(ch)
    d_bins, d_pow = ctx.array((ch, 64, 2), F), ctx.array((ch, 64), F)
    plain = msdr.Chain(ctx, msdr.ARITH_F32, ch, ti[0], tq[0], mixer=msdr.MIXER_NCO, modes=modes, **any_table())
    with pytest.raises(msdr.MsdrError) as e:
        plain.set_spectrum(d_bins, d_pow, 1)
    assert e.value.status == ARG and plain.spectrum() == (None, None, 25, 0)
    plain.close()
    chain, _ = fbank(ctx, ch, 9400)
    for b, p in ((d_bins.offset(8), d_pow), (d_bins, d_pow.offset(4)), (None, d_pow.offset(8))):          # off a 16-byte slot
        with pytest.raises(msdr.MsdrError) as e:
            chain.set_spectrum(b, p, 1)
        assert e.value.status == ARG and chain.spectrum() == (None, None, 25, 0)
    assert ctx.lib.msdr_chain_set_spectrum(None, ctypes.c_void_p(d_bins.ptr), ctypes.c_void_p(d_pow.ptr), 1) == ARG          # a NULL chain
    assert ctx.lib.msdr_chain_get_spectrum(None, None, None, None, None) == ARG
    chain.set_spectrum(d_bins, None, 0)
    assert chain.spectrum() == (d_bins.ptr, None, 25, 0)
    dx = [ctx.to_device(np.zeros((ch, B), np.int16)) for _ in range(2)]
    dy = [ctx.array((ch, B), F) for _ in range(2)]
    with pytest.raises(msdr.MsdrError) as e:          # graphs stay refused, as on every chain in this mode
        chain.graph(dx, dy, B)
    assert e.value.status == ARG
    chain.close()
