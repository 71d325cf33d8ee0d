"""The per-receiver spectrum display of the down-converter bank (Q15): msdr_chain_set_spectrum keeps the most recent 64 pairs behind every
receiver's channel filter and, on showSpectrum's cadence, writes their 64-point transform and its power to buffers of the caller's.

Window tests: the expected bins are the oracle's transform (orc.rfft128_q15's `work`) of tests/spectrum_model.py's tail over the ORACLE's own
pairs (orclib.Oracle.chain_q15(..., want_iq=True)), compared with ==; power against re^2 + im^2 of those bins in int64, reordered.  The
cadence, state and combination tests take the pairs from a caller's d_iq -- tests/test_gpu_iq_per_channel.py holds those to the oracle --
and the same model and transform.  Both output buffers carry a sentinel before every call and a guard row behind the last receiver.
102 taps, off-grid NCO steps, mixed modes; the helpers are those of test_gpu_decim_per_channel.py / test_gpu_iq_per_channel.py."""
import ctypes

import numpy as np
import pytest

import orclib
import spectrum_model as M
from gpuhelp import ctx, msdr  # noqa: F401
from test_gpu_decim_per_channel import nco_chain
from test_gpu_iq_per_channel import bits, padded, pitch_of, sentinel
from test_gpu_nco_per_channel import Bank, any_table, off_grid_steps, u32
from test_gpu_osc_per_channel import lowpass, mixed_bank, notch, oracle_row

pytestmark = pytest.mark.gpu
B = 128
AM, LSB, USB, CW, SYNCAM = orclib.AM, orclib.LSB, orclib.USB, orclib.CW, orclib.SYNCAM
ARG, LEN = msdr.STATUS_ARGUMENT_ERROR, msdr.STATUS_LENGTH_ERROR
SENT32 = 0x7B5A5B5C


class Display:
    """the caller's side of a chain's spectrum: sentinel-filled buffers with a guard row, refilled before every call"""

    def __init__(self, ctx, chain, ch, every=1, bins=True, power=True, dtype=np.int16):
        self.ctx, self.chain, self.ch, self.dtype = ctx, chain, ch, np.dtype(dtype)
        self.pdtype = np.uint32 if self.dtype == np.int16 else np.float32
        self.fresh_b = sentinel((ch + 1, 64, 2), dtype)
        self.fresh_p = np.full((ch + 1, 64), SENT32, np.uint32).view(self.pdtype)
        self.d_bins = ctx.to_device(self.fresh_b) if bins else None
        self.d_pow = ctx.to_device(self.fresh_p) if power else None
        chain.set_spectrum(self.d_bins, self.d_pow, every)

    def arm(self):
        for d, f in ((self.d_bins, self.fresh_b), (self.d_pow, self.fresh_p)):
            if d is not None:
                d.upload(f)

    def read(self):
        """(bins [ch, 64, 2], power [ch, 64]) of a call that drew, (None, None) of one that did not; the guard row is checked either way"""
        b = self.d_bins.download() if self.d_bins is not None else None
        p = self.d_pow.download() if self.d_pow is not None else None
        drew = []
        for got, fresh in ((b, self.fresh_b), (p, self.fresh_p)):
            if got is None:
                continue
            assert np.array_equal(bits(got[self.ch:]), bits(fresh[self.ch:])), "the guard row was written"
            untouched = np.array_equal(bits(got), bits(fresh))
            drew.append(not untouched)
        assert len(set(drew)) == 1, "one buffer was written and the other was not"
        if not drew[0]:
            return None, None
        return (b[:self.ch] if b is not None else None), (p[:self.ch] if p is not None else None)

    def idle(self):
        """the last call wrote neither buffer"""
        b, p = self.read()
        return b is None and p is None


def expect(orc, window):
    """window [ch, 64, 2] int16 -> (bins [ch, 64, 2] int16, power [ch, 64] int64 in display order)"""
    bins = np.stack([M.cfft64_q15(orc, w) for w in window])
    return bins, np.stack([M.power_q15(b) for b in bins])


def check(orc, disp, window, tag):
    got_b, got_p = disp.read()
    assert got_b is not None or got_p is not None, (tag, "no spectrum was drawn")
    want_b, want_p = expect(orc, window)
    if got_b is not None:
        assert np.array_equal(got_b, want_b), (tag, [c for c in range(len(want_b)) if not np.array_equal(got_b[c], want_b[c])])
    if got_p is not None:
        assert np.array_equal(got_p.astype(np.int64), want_p), tag


def call(ctx, chain, xs, D=1, audio=True, dtype=np.int16):
    """one msdr_chain_process over xs [rows, m(, 2)] -> audio [ch, m / D] or None"""
    m = xs.shape[1]
    dy = ctx.array((chain.channels, m // D), dtype) if audio else None
    chain.process(ctx.to_device(np.ascontiguousarray(xs)), dy, m)
    return dy.download() if audio else None


def with_tap(ctx, chain, ch, n_out_max, dtype=np.int16):
    pitch = pitch_of(n_out_max)
    buf = ctx.to_device(sentinel((ch, pitch, 2), dtype))
    chain.set_iq_out(buf, pitch)
    return buf


# ------------------------------------------------------------------------------------------------ 1. the window
WINDOWS = {"a": (1, (128, 768)), "b": (8, (128,) * 6), "c": (3, (72, 192, 3, 390))}


@pytest.mark.parametrize("ch", [1, 5, 17])
@pytest.mark.parametrize("case", sorted(WINDOWS))
def test_the_window_is_the_most_recent_64_pairs(ctx, orc, golden, case, ch):
    """(a) D = 1, calls of 128 and 768: the call's last 64 pairs.  (b) D = 8, six calls of 128 (16 outputs): the last four ticks, the first three
    windows still holding zeros of the cleared tail.  (c) D = 3, n_out = 24, 64, 1, 130.  every = 1, checked after every call, on three
    chains: spectrum alone (the chain's own pair buffer), spectrum beside a caller's d_iq, and no spectrum at all."""
    D, calls = WINDOWS[case]
    rng = np.random.default_rng(8100 + ch + 100 * D)
    n = sum(calls)
    n128 = (n + B - 1) // B * B
    modes, ti, tq = mixed_bank(golden, ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    si, sq = Bank(steps, phases).advance(n128)
    x = rng.integers(-30000, 30001, (ch, n)).astype(np.int16)
    want = [oracle_row(orc, padded(x[c], n128), si[c], sq[c], lambda b: (modes[c], ti[c], tq[c]), {}, want_iq=True) for c in range(ch)]
    audio_w = np.stack([w[0][D - 1:n:D] for w in want])
    pairs_w = np.stack([np.stack([w[1][D - 1:n:D], w[2][D - 1:n:D]], axis=1) for w in want])          # [ch, n / D, 2]
    alone, tapped, plain = (nco_chain(ctx, ch, ti, tq, steps, phases, modes) for _ in range(3))
    for c in (alone, tapped, plain):
        c.channels = ch
        if D > 1:
            c.set_decimation(D)
    d_alone, d_tapped = Display(ctx, alone, ch), Display(ctx, tapped, ch)
    buf = with_tap(ctx, tapped, ch, max(calls) // D)
    tail, lo = M.Tail(ch), 0
    for k, m in enumerate(calls):
        xs, o = x[:, lo:lo + m], slice(lo // D, (lo + m) // D)
        window = tail.push(pairs_w[:, o])
        if case == "b" and k < 3:
            assert not window[:, :64 - 16 * (k + 1)].any() and window[:, -16:].any()
        for chain, disp in ((alone, d_alone), (tapped, d_tapped)):
            disp.arm()
            got = call(ctx, chain, xs, D)
            assert np.array_equal(got, audio_w[:, o]), (case, k)
            check(orc, disp, window, (case, k))
            assert chain.spectrum()[2:] == (1, k + 1)
        assert np.array_equal(buf.download()[:, :m // D], pairs_w[:, o]), (case, k)
        assert np.array_equal(call(ctx, plain, xs, D), audio_w[:, o]), (case, k)
        lo += m
    assert alone.info()["kernel"] == plain.info()["kernel"]          # the names stay
    for c in (alone, tapped, plain):
        c.close()


# ------------------------------------------------------------------------------------------------ 2. the cadence
def bank(ctx, golden, ch, seed, D=8, zero_phase=False, **kw):
    rng = np.random.default_rng(seed)
    modes, ti, tq = mixed_bank(golden, ch)
    steps = off_grid_steps(rng, ch)
    phases = np.zeros(ch, np.uint64) if zero_phase else rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    chain = nco_chain(ctx, ch, ti, tq, steps, phases, modes, **kw)
    chain.channels = ch
    if D > 1:
        chain.set_decimation(D)
    return chain, rng


def tick(ctx, chain, buf, tail, rng, D=8, m=B, audio=True):
    """one call of m fresh samples; the window behind it from the device's own pairs"""
    x = rng.integers(-30000, 30001, (chain.channels, m)).astype(np.int16)
    got = call(ctx, chain, x, D, audio)
    return tail.push(buf.download()[:, :m // D]), got, x


@pytest.mark.parametrize("every, calls, draws", [(3, 8, (0, 3, 6)), (0, 27, (0, 25)), (1, 4, (0, 1, 2, 3))])
def test_the_cadence_is_showspectrums(ctx, orc, golden, every, calls, draws):
    ch = 5
    chain, rng = bank(ctx, golden, ch, 8200 + every)
    buf = with_tap(ctx, chain, ch, 16)
    disp, tail, model = Display(ctx, chain, ch, every), M.Tail(ch), M.Tick(every)
    for k in range(calls):
        disp.arm()
        window, _, _ = tick(ctx, chain, buf, tail, rng)
        assert model.tick() == (k in draws)
        if k in draws:
            check(orc, disp, window, k)
        else:
            assert disp.idle(), k          # a call that does not draw writes neither buffer
        assert chain.spectrum() == (disp.d_bins.ptr, disp.d_pow.ptr, every or 25, model.drawn)
    assert chain.spectrum()[3] == len(draws)
    chain.close()


def test_another_every_while_on_keeps_the_counter(ctx, orc, golden):
    """every = 3; behind call 0 the counter holds 3.  every = 5 set then: the next spectrum is still call 3's, the one after it call 8's.  Other
    pointers while on: tail, counter and count stay."""
    ch = 5
    chain, rng = bank(ctx, golden, ch, 8300)
    buf = with_tap(ctx, chain, ch, 16)
    disp, tail = Display(ctx, chain, ch, 3), M.Tail(ch)
    drew = []
    for k in range(10):
        if k == 1:
            chain.set_spectrum(disp.d_bins, disp.d_pow, 5)
        if k == 2:          # power only from here on
            chain.set_spectrum(None, disp.d_pow, 5)
            disp.d_bins = None
            assert chain.spectrum()[0] is None and chain.spectrum()[3] == 1
        disp.arm()
        window, _, _ = tick(ctx, chain, buf, tail, rng)
        if not disp.idle():
            drew.append(k)
            check(orc, disp, window, k)
    assert drew == [0, 3, 8] and chain.spectrum()[2:] == (5, 3)
    chain.close()


# ------------------------------------------------------------------------------------------------ 3. state
def test_off_to_on_reset_init_fir_and_a_failed_call(ctx, orc, golden):
    ch = 5
    chain, rng = bank(ctx, golden, ch, 8400, zero_phase=True)
    buf = with_tap(ctx, chain, ch, 16)
    disp, tail = Display(ctx, chain, ch, 2), M.Tail(ch)
    disp.arm()
    check(orc, disp, tick(ctx, chain, buf, tail, rng)[0], "call 0")
    disp.arm()
    tick(ctx, chain, buf, tail, rng)
    assert disp.idle() and chain.spectrum()[3] == 1
    # off -> on: tail, counter and count start over -- the next call draws zeros ++ its own 16 pairs
    chain.set_spectrum(None, None)
    assert chain.spectrum()[:2] == (None, None)
    disp.arm()
    call(ctx, chain, rng.integers(-30000, 30001, (ch, B)).astype(np.int16), 8)          # a call while off: nothing written, nothing kept
    assert disp.idle()
    chain.set_spectrum(disp.d_bins, disp.d_pow, 2)
    assert chain.spectrum()[3] == 0
    tail.clear()
    disp.arm()
    window = tick(ctx, chain, buf, tail, rng)[0]
    assert not window[:, :48].any()
    check(orc, disp, window, "off -> on")
    assert chain.spectrum()[3] == 1
    disp.arm()
    tick(ctx, chain, buf, tail, rng)
    assert disp.idle()          # counter 2 -> 1
    # a LENGTH_ERROR call (n % D != 0) changes nothing
    disp.arm()
    with pytest.raises(msdr.MsdrError) as e:
        chain.process(ctx.to_device(np.zeros((ch, 100), np.int16)), ctx.array((ch, 12), np.int16), 100)
    assert e.value.status == LEN and disp.idle() and chain.spectrum()[3] == 1
    disp.arm()
    check(orc, disp, tick(ctx, chain, buf, tail, rng)[0], "behind the failed call")          # counter 1 -> draws, the model's window
    assert chain.spectrum()[3] == 2
    # init_fir keeps tail and counter: the next call does not draw, the one after it draws a window that reaches back across init_fir
    chain.init_fir()
    disp.arm()
    tick(ctx, chain, buf, tail, rng)
    assert disp.idle()
    disp.arm()
    window = tick(ctx, chain, buf, tail, rng)[0]
    check(orc, disp, window, "across init_fir")
    assert window[:, :32].any()
    # reset clears tail and counter (the count goes on): the next call draws zeros ++ its own pairs
    disp.arm()
    tick(ctx, chain, buf, tail, rng)
    assert disp.idle()
    chain.reset()
    tail.clear()
    disp.arm()
    window = tick(ctx, chain, buf, tail, rng)[0]
    assert not window[:, :48].any()
    check(orc, disp, window, "behind reset")
    assert chain.spectrum()[3] == 4
    chain.close()


# ------------------------------------------------------------------------------------------------ 4. combinations
def twin_run(ctx, orc, make, calls=4, D=8, m=B, audio_of=lambda k: True, pll=(), xshape=None, every=1, amp=20000):
    """the same calls on make() with the spectrum on (no d_iq unless make sets one) and on make() with a d_iq and no spectrum: audio, meter and
    PLL state equal, the spectrum the model's over the second chain's pairs"""
    on, off = make(), make()
    ch = on.channels
    has_tap = on.iq_out()[0] is not None
    buf = with_tap(ctx, off, ch, m // D) if not has_tap else off._iq_out
    disp, tail = Display(ctx, on, ch, every), M.Tail(ch)
    rng = np.random.default_rng(8500)
    meters = []
    for c in (on, off):
        if c.meter() is not None:
            meters.append(c._meter)
    for k in range(calls):
        x = rng.integers(-amp, amp + 1, xshape(ch, m) if xshape else (ch, m)).astype(np.int16)
        disp.arm()
        a_on, a_off = call(ctx, on, x, D, audio_of(k)), call(ctx, off, x, D, audio_of(k))
        if audio_of(k):
            assert np.array_equal(a_on, a_off), k
        if meters:
            assert np.array_equal(meters[0].download(), meters[1].download()) and meters[0].download().any(), k
        for c in pll:
            assert np.array_equal(on.pll_state(c).view(np.uint32), off.pll_state(c).view(np.uint32)), (k, c)
        window = tail.push(buf.download()[:, :m // D])
        if has_tap:
            assert np.array_equal(on._iq_out.download()[:, :m // D], buf.download()[:, :m // D]), k
        check(orc, disp, window, k)
    kernels = on.info()["kernel"], off.info()["kernel"]
    on.close(); off.close()
    return window, kernels


def test_with_the_meter(ctx, orc, golden):
    def make():
        chain, _ = bank(ctx, golden, 5, 8510)
        chain.set_meter(ctx.to_device(np.zeros(5, np.uint64)))
        return chain
    twin_run(ctx, orc, make)


def test_with_gain_the_spectrum_sees_the_gained_pairs(ctx, orc, golden):
    def make(gain=4.0):
        chain, _ = bank(ctx, golden, 5, 8520)
        chain.set_meter(ctx.to_device(np.zeros(5, np.uint64)))
        chain.set_gain(True)
        chain.set_gain_channels(2, np.array([gain], np.float32))
        return chain
    gained, _ = twin_run(ctx, orc, make, m=8 * B, amp=2000)          # (small enough that four times the pair stays inside int16)
    unity, _ = twin_run(ctx, orc, lambda: make(1.0), m=8 * B, amp=2000)
    g, u = gained.astype(np.int64), unity.astype(np.int64)
    assert np.array_equal(g[[0, 1, 3, 4]], u[[0, 1, 3, 4]])
    big = np.abs(u[2]) > 100
    assert big.any() and np.abs(u[2]).max() < 8000 and np.abs(g[2][big] - 4 * u[2][big]).max() <= 4          # receiver 2 alone, four times as large


def test_on_complex_input(ctx, orc, golden):
    def make():
        chain, _ = bank(ctx, golden, 5, 8530)
        chain.set_complex_input(True, 0)
        return chain
    twin_run(ctx, orc, make, xshape=lambda ch, m: (ch, m, 2))


def test_on_a_shared_antenna_row(ctx, orc, golden):
    def make():
        chain, _ = bank(ctx, golden, 5, 8540)
        chain.set_input_rows(np.zeros(5, np.int64), 1)
        return chain
    twin_run(ctx, orc, make, xshape=lambda ch, m: (1, m))


def test_beside_the_banks_pll(ctx, orc, golden):
    def make():
        modes, ti, tq = mixed_bank(golden, 5)
        modes[1] = SYNCAM
        rng = np.random.default_rng(8550)
        chain = msdr.Chain(ctx, msdr.ARITH_Q15, 5, ti[0], tq[0], mixer=msdr.MIXER_NCO, modes=modes, flags=msdr.CHAIN_SYNCAM_PLL, **any_table())
        chain.set_bank_post(True)
        chain.set_taps_channels(0, ti, tq)
        chain.set_nco_channels(0, u32(off_grid_steps(rng, 5)), u32(rng.integers(0, 1 << 32, 5, dtype=np.uint64)))
        chain.set_decimation(8)
        chain.channels = 5
        return chain
    twin_run(ctx, orc, make, pll=(1,))


def test_iq_only_calls_feed_the_window(ctx, orc, golden):
    def make():
        chain, _ = bank(ctx, golden, 5, 8560)
        with_tap(ctx, chain, 5, 16)
        return chain
    twin_run(ctx, orc, make, calls=6, audio_of=lambda k: k % 2 == 1)


def test_with_per_channel_nodes_behind_it(ctx, orc, golden):
    def make():
        chain, _ = bank(ctx, golden, 5, 8570, biquad_nodes=[[lowpass()], [notch(0)]])
        chain.set_node_coefficients_channels(1, 0, 0, np.stack([notch(c) for c in range(5)]))
        return chain
    _, kernels = twin_run(ctx, orc, make)
    assert kernels[0] == kernels[1]


def test_with_the_block_kernel_switch_on(ctx, orc, golden):
    def make():
        chain, _ = bank(ctx, golden, 5, 8580, D=1)
        chain.set_block_kernel_q15(1)
        return chain
    _, kernels = twin_run(ctx, orc, make, D=1)
    assert kernels[0] == kernels[1] and kernels[0].startswith("chain_q15pcn_kernel")          # the unfused launches, as with the meter


# ------------------------------------------------------------------------------------------------ 5. refusals
def test_refusals_change_nothing(ctx, golden):
    ch = 5
    modes, ti, tq = mixed_bank(golden, ch)
    d_bins, d_pow = ctx.to_device(sentinel((ch + 1, 64, 2), np.int16)), ctx.to_device(np.full((ch + 1, 64), SENT32, np.uint32))
    plain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, ti[0], tq[0], mixer=msdr.MIXER_NCO, modes=modes, **any_table())
    with pytest.raises(msdr.MsdrError) as e:          # not in phase-accumulator mode
        plain.set_spectrum(d_bins, d_pow, 1)
    assert e.value.status == ARG and plain.spectrum() == (None, None, 25, 0)
    plain.close()
    chain, rng = bank(ctx, golden, ch, 8600, D=1)
    for b, p in ((d_bins.offset(8), d_pow), (d_bins, d_pow.offset(4))):
        with pytest.raises(msdr.MsdrError) as e:
            chain.set_spectrum(b, p, 1)
        assert e.value.status == ARG and chain.spectrum() == (None, None, 25, 0)
    lib = ctx.lib
    assert lib.msdr_chain_set_spectrum(None, ctypes.c_void_p(d_bins.ptr), None, 1) == ARG
    chain.set_spectrum(d_bins, d_pow, 7)
    assert chain.spectrum() == (d_bins.ptr, d_pow.ptr, 7, 0)
    dx = [ctx.to_device(np.zeros((ch, B), np.int16)) for _ in range(2)]
    dy = [ctx.array((ch, B), np.int16) for _ in range(2)]
    with pytest.raises(msdr.MsdrError) as e:          # graphs stay refused, as on every chain in this mode
        chain.graph(dx, dy, B)
    assert e.value.status == ARG and chain.spectrum() == (d_bins.ptr, d_pow.ptr, 7, 0)
    ctx.synchronize()
    assert (d_pow.download() == SENT32).all()
    chain.close()
