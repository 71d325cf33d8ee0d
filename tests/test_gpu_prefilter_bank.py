"""What sits behind the FIR accumulators of the down-converter bank, behind the two-stage kernel at (D1, N1, D2) = (4, 16, 4): the S-meter, the
pairs, a gained receiver with its AGC (tests/agc_model.py), the bank's PLL at set_pll_rate(fs / 16) (tests/pll_model.py), the spectrum tail
(tests/spectrum_model.py) and per-channel nodes at the final rate.  All of it counts its rate as fs / (D1 D2) and sees n_samples / (D1 D2)
outputs per call.  Q15: everything is compared with ==; the fp32 meter is held to tests/test_gpu_meter_per_channel_f32.py's 2.5e-5.  Audio,
pairs and meter with each extra on are bit-identical to the two-stage chain without it."""
import numpy as np
import pytest

import agc_model as agc
import orclib
import pll_model
import prefilter_model as pm
import spectrum_model as sm
from gpuhelp import ctx, msdr  # noqa: F401
from test_gpu_nco_per_channel import Bank, any_table, u32
from test_gpu_osc_per_channel import bw_taps, lowpass, notch, pad

pytestmark = pytest.mark.gpu
FS = 24000.0
D1, N1, D2 = 4, 16, 4
DD = D1 * D2
CH = 10
NOUTS = (96, 8, 72)
TOTAL = sum(NOUTS)
PITCH = 104
AM, LSB, USB, CW, SYNCAM = orclib.AM, orclib.LSB, orclib.USB, orclib.CW, orclib.SYNCAM
I16 = np.int16


@pytest.fixture(scope="module")
def ref(orc, golden):
    """the bank on one antenna row: per receiver the stage-2 ACCUMULATORS of every output (tests/agc_model.py: arm_fir_fast_q15's before its
    >> 15) over the oracle's stage-1 intermediates, and the plain pair and audio they give"""
    rng = np.random.default_rng(7300)
    modes = np.array([(AM, SYNCAM, USB, LSB, CW)[c % 5] for c in range(CH)], np.int32)
    ti = np.stack([bw_taps(1500.0 + 90.0 * c) if modes[c] in (AM, SYNCAM) else pad(golden["taps/FIR_CW_I_coeffs" if modes[c] == CW else "taps/FIR_SSB_I_coeffs"]) for c in range(CH)])
    tq = np.stack([ti[c] if modes[c] in (AM, SYNCAM) else pad(golden["taps/FIR_CW_Q_coeffs" if modes[c] == CW else "taps/FIR_SSB_Q_coeffs"]) for c in range(CH)])
    steps = rng.integers(1, 1 << 32, CH, dtype=np.uint64) | np.uint64(1)
    sync = np.flatnonzero(modes == SYNCAM)
    steps[sync] = np.array([msdr.nco_step(500.0 + 700.0 * k, FS) for k in range(sync.size)], np.uint64) | np.uint64(1)
    phases = rng.integers(0, 1 << 32, CH, dtype=np.uint64)
    n = TOTAL * DD
    t = np.arange(n)
    f_rx = steps[sync].astype(np.float64) / 2.0 ** 32 * FS
    carriers = sum((1 + 0.4 * np.sin(2 * np.pi * (15.0 + 3.0 * k) * t / FS)) * np.cos(2 * np.pi * (f + 20.0) * t / FS + 0.3 * k) for k, f in enumerate(f_rx))
    x = np.round(5000.0 * carriers + rng.normal(0, 2500, n)).astype(I16)
    si, sq = Bank(steps, phases).advance(n)
    p = pm.lowpass(D1, N1, I16)
    acc, plain, audio = [], [], []
    for c in range(CH):
        mi, mq = agc.mixed_q15(orc, x, None, si[c], sq[c], 1)
        rc, ui = orc.fir_q15_blocks(p, mi, 128)
        assert rc == 0
        rc, uq = orc.fir_q15_blocks(p, mq, 128)
        assert rc == 0
        ai, aq = agc.acc_q15(ui[D1 - 1::D1], ti[c])[D2 - 1::D2], agc.acc_q15(uq[D1 - 1::D1], tq[c])[D2 - 1::D2]
        acc.append((ai, aq))
        plain.append(np.stack([agc.plain_q15(ai), agc.plain_q15(aq)], -1))
        a, fi, fq = pm.model_q15(orc, x, si[c], sq[c], p, D1, modes[c], ti[c], tq[c], D2)
        assert np.array_equal(plain[c][:, 0], fi) and np.array_equal(plain[c][:, 1], fq)          # (the two statements of the model agree)
        audio.append(a)
    return dict(modes=modes, ti=ti, tq=tq, steps=steps, phases=phases, x=x, p=p, acc=acc, plain=np.stack(plain), audio=np.stack(audio), sync=sync)


def make_chain(ctx, ref, modes=None, **kw):
    modes = ref["modes"] if modes is None else modes
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, CH, ref["ti"][0], ref["tq"][0], mixer=msdr.MIXER_NCO, modes=modes, **any_table(), **kw)
    if kw.get("flags", 0) & msdr.CHAIN_SYNCAM_PLL:
        chain.set_bank_post(True)
    chain.set_taps_channels(0, ref["ti"], ref["tq"])
    chain.set_nco_channels(0, u32(ref["steps"]), u32(ref["phases"]))
    chain.set_input_rows(np.zeros(CH, np.int64), 1)
    chain.set_prefilter(D1, ref["p"])
    chain.set_decimation(D2)
    return chain


def run_calls(ctx, chain, ref, iq=False, meter=False, after=None):
    """the three calls -> (audio [CH, TOTAL], pairs [CH, TOTAL, 2] or None, meters [calls, CH] or None); after(call, lo, nout) runs behind each"""
    audio = np.empty((CH, TOTAL), I16)
    pairs = np.empty((CH, TOTAL, 2), I16) if iq else None
    meters = []
    buf = met = None
    if iq:
        buf = ctx.to_device(np.zeros((CH, PITCH, 2), I16))
        chain.set_iq_out(buf, PITCH)
    if meter:
        met = ctx.to_device(np.zeros(CH, np.uint64))
        chain.set_meter(met)
    lo = 0
    for k, nout in enumerate(NOUTS):
        dy = ctx.array((CH, nout), I16)
        chain.process(ctx.to_device(np.ascontiguousarray(ref["x"][None, lo * DD:(lo + nout) * DD])), dy, nout * DD)
        audio[:, lo:lo + nout] = dy.download()
        if iq:
            pairs[:, lo:lo + nout] = buf.download()[:, :nout]
        if meter:
            meters.append(met.download().copy())
        if after:
            after(k, lo, nout)
        lo += nout
    assert chain.info()["kernel"].startswith("chain_q15pcn2_kernel"), chain.info()
    return audio, pairs, (np.stack(meters) if meter else None)


def no_sync(ref):
    return np.where(ref["modes"] == SYNCAM, AM, ref["modes"]).astype(np.int32)


@pytest.fixture(scope="module")
def plain(ctx, ref):
    """the two-stage chain without any extra (SYNCAM channels as AM: no PLL on this chain)"""
    chain = make_chain(ctx, ref, modes=no_sync(ref))
    audio, _, _ = run_calls(ctx, chain, ref)
    chain.close()
    return audio


def expected_audio(orc, ref, modes):
    return np.stack([ref["audio"][c] if modes[c] == ref["modes"][c] else orc.demod_q15(int(modes[c]), ref["plain"][c, :, 0], ref["plain"][c, :, 1]) for c in range(CH)])


def test_the_plain_chain_is_the_model(orc, ref, plain):
    assert np.array_equal(plain, expected_audio(orc, ref, no_sync(ref)))
    assert np.abs(plain.astype(np.int32)).max() > 1000


def test_meter_and_pairs(ctx, orc, ref, plain):
    chain = make_chain(ctx, ref, modes=no_sync(ref))
    audio, pairs, meters = run_calls(ctx, chain, ref, iq=True, meter=True)
    chain.close()
    assert np.array_equal(audio, plain)
    assert np.array_equal(pairs, ref["plain"])
    lo = 0
    for k, nout in enumerate(NOUTS):
        want = (ref["plain"][:, lo:lo + nout].astype(np.int64) ** 2).sum(axis=(1, 2)).astype(np.uint64)
        assert np.array_equal(meters[k], want), k
        lo += nout


def test_a_gained_receiver_and_its_agc(ctx, orc, ref, plain):
    modes = no_sync(ref)
    gains = np.array([0.25, 1.0, 3.0, -2.5, 1.0, 0.5, 1.0, 40.0, 1.0, 0.0], np.float32)
    on = np.array([1, 0, 1, 0, 0, 1, 1, 0, 0, 1], np.int32)
    # gain on, every gain 1.0, AGC off: no output bit changes
    chain = make_chain(ctx, ref, modes=modes)
    chain.set_gain(True)
    audio, pairs, meters = run_calls(ctx, chain, ref, iq=True, meter=True)
    assert np.array_equal(audio, plain) and np.array_equal(pairs, ref["plain"])
    chain.close()
    chain = make_chain(ctx, ref, modes=modes)
    chain.set_gain(True)
    chain.set_gain_channels(0, gains)
    chain.set_agc(on)
    rxs = [agc.Rx() for _ in range(CH)]
    for c, rx in enumerate(rxs):
        rx.set_gain(gains[c])
        rx.on = int(on[c])
    want_audio, want_pairs = np.empty((CH, TOTAL), I16), np.empty((CH, TOTAL, 2), I16)

    def after(k, lo, nout):
        for c, rx in enumerate(rxs):
            gi, gq = agc.pair_q15(ref["acc"][c][0][lo:lo + nout], rx.mult), agc.pair_q15(ref["acc"][c][1][lo:lo + nout], rx.mult)
            want_pairs[c, lo:lo + nout, 0], want_pairs[c, lo:lo + nout, 1] = gi, gq
            want_audio[c, lo:lo + nout] = orc.demod_q15(int(modes[c]), gi, gq)
            rx.after_call(rx.absmax_of(gi, gq))
        agc.check_words(chain, rxs, "call %d" % k)

    audio, pairs, meters2 = run_calls(ctx, chain, ref, iq=True, meter=True, after=after)
    chain.close()
    assert np.array_equal(pairs, want_pairs) and np.array_equal(audio, want_audio)
    assert np.array_equal(meters2, meters)          # the meter keeps the ungained pair
    assert any(rx.steps for rx in rxs) and not np.array_equal(audio, plain)


def test_the_bank_pll_at_the_final_rate(ctx, orc, ref):
    k = msdr.syncam_constants_rate(FS / DD)
    chain = make_chain(ctx, ref, flags=msdr.CHAIN_SYNCAM_PLL)
    chain.set_pll_rate(FS / DD)
    plls = {c: pll_model.Pll(k) for c in ref["sync"]}
    want = ref["audio"].copy()

    def after(call, lo, nout):
        for c, pll in plls.items():
            want[c, lo:lo + nout] = pll.run_q15(ref["plain"][c, lo:lo + nout, 0], ref["plain"][c, lo:lo + nout, 1])
            assert np.array_equal(chain.pll_state(c).view(np.uint32), pll.state().view(np.uint32)), (call, c)

    audio, pairs, _ = run_calls(ctx, chain, ref, iq=True, after=after)
    assert chain.post_kernel() == "bank_pll_q15_kernel"
    chain.close()
    assert np.array_equal(pairs, ref["plain"])
    bad = [c for c in range(CH) if not np.array_equal(audio[c], want[c])]
    assert not bad, bad
    # the constants matter: the reference's give another audio on the SYNCAM receivers
    o = orc.syncam_new()
    c0 = int(ref["sync"][0])
    assert not np.array_equal(orc.syncam_q15(o, ref["plain"][c0, :NOUTS[0], 0], ref["plain"][c0, :NOUTS[0], 1]), want[c0, :NOUTS[0]])


def test_the_spectrum_tail(ctx, orc, ref, plain):
    chain = make_chain(ctx, ref, modes=no_sync(ref))
    d_bins, d_pow = ctx.to_device(np.zeros((CH, 64, 2), I16)), ctx.to_device(np.zeros((CH, 64), np.uint32))
    chain.set_spectrum(d_bins, d_pow, 1)          # every call draws
    tail = sm.Tail(CH)

    def after(k, lo, nout):
        w = tail.push(ref["plain"][:, lo:lo + nout])
        bins = np.stack([sm.cfft64_q15(orc, w[c]) for c in range(CH)])
        assert np.array_equal(d_bins.download(), bins), k
        assert np.array_equal(d_pow.download().astype(np.int64), np.stack([sm.power_q15(b) for b in bins])), k

    audio, _, _ = run_calls(ctx, chain, ref, after=after)
    assert chain.spectrum()[3] == len(NOUTS)
    chain.close()
    assert np.array_equal(audio, plain)


def test_per_channel_nodes_at_the_final_rate(ctx, orc, ref, plain):
    modes = no_sync(ref)
    chain = make_chain(ctx, ref, modes=modes, biquad_nodes=[[lowpass()], [lowpass()]])
    chain.set_node_coefficients_channels(0, 0, 0, np.stack([lowpass() for _ in range(CH)]))
    chain.set_node_coefficients_channels(1, 0, 0, np.stack([notch(c) for c in range(CH)]))
    audio, _, _ = run_calls(ctx, chain, ref)
    chain.close()
    for c in range(CH):
        bq = [orc.biquad_teensy_new([lowpass()]), orc.biquad_teensy_new([notch(c)])]
        lo, want = 0, []
        for nout in NOUTS:
            seg = plain[c, lo:lo + nout].copy()
            for b in bq:
                seg = orc.biquad_teensy_update(b, seg)
            want.append(seg)
            lo += nout
        assert np.array_equal(audio[c], np.concatenate(want)), c


def test_the_fp32_meter_and_pairs(ctx, orc):
    """fp32: the meter within 2.5e-5 of the oracle's sum of squares, and audio, pairs and meter bit-identical whichever of the extras is on"""
    from test_gpu_osc_per_channel_f32 import mixed_bank, signal
    F = np.float32
    rng = np.random.default_rng(7301)
    ch = 7
    modes, ti, tq = mixed_bank(ch)
    steps, phases = rng.integers(1, 1 << 32, ch, dtype=np.uint64), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    p = pm.lowpass(D1, N1, F)
    x = signal(rng, ch, TOTAL * DD)
    si, sq = Bank(steps, phases).advance(TOTAL * DD)
    want = [pm.model_f32(orc, x[c], si[c], sq[c], p, D1, modes[c], ti[c], tq[c], D2) for c in range(ch)]
    runs = {}
    for tag in ("plain", "meter", "iq", "both", "gain"):
        chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, ti[0], tq[0], mixer=msdr.MIXER_NCO, modes=modes, **any_table())
        chain.set_taps_channels_f32(0, ti, tq)
        chain.set_nco_channels(0, u32(steps), u32(phases))
        chain.set_prefilter(D1, p)
        chain.set_decimation(D2)
        met = buf = None
        if tag in ("meter", "both", "gain"):
            met = ctx.to_device(np.zeros(ch, np.float64))
            chain.set_meter(met)
        if tag in ("iq", "both", "gain"):
            buf = ctx.to_device(np.zeros((ch, PITCH, 2), F))
            chain.set_iq_out(buf, PITCH)
        if tag == "gain":
            chain.set_gain(True)
        audio, pairs, meters, lo = [], [], [], 0
        for nout in NOUTS:
            dy = ctx.array((ch, nout), F)
            chain.process(ctx.to_device(np.ascontiguousarray(x[:, lo * DD:(lo + nout) * DD])), dy, nout * DD)
            audio.append(dy.download())
            pairs.append(buf.download()[:, :nout].copy() if buf is not None else None)
            meters.append(met.download().copy() if met is not None else None)
            lo += nout
        info = chain.info()
        assert info["kernel"].startswith("chain_f32pcn2_kernel") and info["flavour"] & msdr.FLAVOUR_PREFILTER, info
        assert bool(info["flavour"] & msdr.FLAVOUR_METER) == (met is not None) and bool(info["flavour"] & msdr.FLAVOUR_IQ_OUT) == (buf is not None), info
        runs[tag] = (np.concatenate(audio, 1), pairs, meters)
        chain.close()
    for tag in ("meter", "iq", "both", "gain"):
        assert np.array_equal(runs[tag][0].view(np.uint32), runs["plain"][0].view(np.uint32)), tag
    for k in range(len(NOUTS)):
        assert np.array_equal(runs["iq"][1][k].view(np.uint32), runs["both"][1][k].view(np.uint32)) and np.array_equal(runs["gain"][1][k].view(np.uint32), runs["both"][1][k].view(np.uint32))
        assert np.array_equal(runs["meter"][2][k], runs["both"][2][k]) and np.array_equal(runs["gain"][2][k], runs["both"][2][k])
    lo = 0
    for k, nout in enumerate(NOUTS):
        for c in range(ch):
            fi, fq = (want[c][j][lo:lo + nout].astype(np.float64) for j in (1, 2))
            w = float((fi * fi + fq * fq).sum())
            got = runs["both"][2][k][c]
            print("prefilter f32 meter call %d ch %d rel %.3e" % (k, c, abs(got - w) / w))
            assert abs(got - w) <= 2.5e-5 * w, (k, c)
        lo += nout
