"""GPU parity of the fused chain (msdr_chain_*) through the C ABI.

q15 arithmetic: bit-exact against the reference-generated golden vectors and the oracle.
fp32 arithmetic: relative RMS <= 1e-5 per channel against the oracle's sequential fp32 chain
(BASELINE.json north_star: "demodulated audio within 1e-5 RMS of the CMSIS reference")."""
import numpy as np
import pytest

import orclib
from gpuhelp import ctx, msdr, rel_rms  # noqa: F401

pytestmark = pytest.mark.gpu
B = 128
TOL = 1e-5
CORR = orclib.AUDIO_SAMPLE_RATE_EXACT / 24000.0

CHAIN = [("AM", orclib.AM, "fir/taps_am102", "fir/taps_am102"),
         ("LSB", orclib.LSB, "taps/FIR_SSB_I_coeffs", "taps/FIR_SSB_Q_coeffs"),
         ("USB", orclib.USB, "taps/FIR_SSB_I_coeffs", "taps/FIR_SSB_Q_coeffs"),
         ("CW", orclib.CW, "taps/FIR_CW_I_coeffs", "taps/FIR_CW_Q_coeffs")]


def run_chain(ctx, chain, x, out_dtype, block=None, node_kernel=None):
    """x: [channels, n] int16. block=None -> one call; else consecutive calls of `block` samples.
    node_kernel: what Chain.node_kernel() must report after every call (the kernel that ran the biquad nodes)."""
    ch, n = x.shape
    out = np.empty((ch, n), out_dtype)
    step = block or n
    for o in range(0, n, step):
        m = min(step, n - o)
        dx, dy = ctx.to_device(x[:, o:o + m]), ctx.array((ch, m), out_dtype)
        chain.process(dx, dy, m)
        if node_kernel is not None:
            assert chain.node_kernel() == node_kernel, (o, m, chain.node_kernel(), chain.info()["kernel"])
        out[:, o:o + m] = dy.download()
    return out


# ---------------------------------------------------------------- q15: golden --------------
@pytest.mark.parametrize("mn,mode,ti,tq", CHAIN)
@pytest.mark.parametrize("block", [128, None])
def test_chain_q15_matches_reference_golden(ctx, golden, mn, mode, ti, tq, block):
    sigs = ["am", "tones", "noise", "full"]
    x = np.stack([golden["chain/x_" + s] for s in sigs])
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, len(sigs), golden[ti], golden[tq], mode=mode)
    got = run_chain(ctx, chain, x, np.int16, block)
    for c, s in enumerate(sigs):
        assert np.array_equal(got[c], golden["chain/%s_%s_audio" % (s, mn)]), (s, mn, block)
    if mn in ("AM", "CW"):
        chain2 = msdr.Chain(ctx, msdr.ARITH_Q15, len(sigs), golden[ti], golden[tq], mode=mode, sqrt_kind=msdr.SQRT_Q31)
        got = run_chain(ctx, chain2, x, np.int16, block)
        for c, s in enumerate(sigs):
            assert np.array_equal(got[c], golden["chain/%s_%s_audio_q31" % (s, mn)]), (s, mn)


def _ref_nodes(orc):
    lp = orc.biquad_design(orclib.BQ_LOWPASS, np.float32(6000 * 0.9 * CORR), 0.54)       # .ino:391-393
    nt = orc.biquad_design(orclib.BQ_NOTCH, np.float32(24000 / 8 * CORR), 15.0)           # .ino:356
    return lp, nt


def test_chain_q15_reference_graph_mixed_modes(ctx, orc, golden):
    """demodulation() + biquad1_dac (LP) + biquad2_dac (notch), per-channel mode and tap set (C5 shape)."""
    lp, nt = _ref_nodes(orc)
    rng = np.random.default_rng(30)
    ch, n = 9, 24 * B
    x = rng.integers(-12000, 12001, (ch, n)).astype(np.int16)
    modes = np.array([orclib.AM, orclib.LSB, orclib.USB, orclib.CW, orclib.AM, orclib.LSB, orclib.USB, orclib.CW, orclib.AM], np.int32)
    am = np.concatenate([golden["fir/taps_am102"]])                      # 102 taps
    pad = lambda t: np.concatenate([np.zeros(102 - t.size, np.int16), t])   # front zero-padding = same filter
    sets_i = [am, pad(golden["taps/FIR_SSB_I_coeffs"]), pad(golden["taps/FIR_CW_I_coeffs"])]
    sets_q = [am, pad(golden["taps/FIR_SSB_Q_coeffs"]), pad(golden["taps/FIR_CW_Q_coeffs"])]
    which = {orclib.AM: 0, orclib.LSB: 1, orclib.USB: 1, orclib.CW: 2}
    tapsets = np.array([which[m] for m in modes], np.int32)
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, sets_i, sets_q, modes=modes, tapsets=tapsets, biquad_nodes=[[lp], [nt]])
    for block in (128, 5 * B):
        chain.reset()
        nodes_fresh = msdr.Chain(ctx, msdr.ARITH_Q15, ch, sets_i, sets_q, modes=modes, tapsets=tapsets,
                                 biquad_nodes=[[lp], [nt]])
        got = run_chain(ctx, nodes_fresh, x, np.int16, block)
        for c in range(ch):
            want = orc.chain_q15(x[c], modes[c], sets_i[tapsets[c]], sets_q[tapsets[c]],
                                 biquads=[orc.biquad_teensy_new([lp]), orc.biquad_teensy_new([nt])])
            assert np.array_equal(got[c], want), (block, c)


def test_chain_q15_nco_mixer_and_long_block(ctx, orc, golden):
    """AudioEffectFreqConv front end (freq_conv.cpp) + a long block that the GPU splits in time."""
    n = np.arange(B)
    oi = np.round(32767 * np.sin(2 * np.pi * 32 * n / B)).astype(np.int16)
    oq = np.round(32767 * np.cos(2 * np.pi * 32 * n / B)).astype(np.int16)
    rng = np.random.default_rng(31)
    x = rng.integers(-32768, 32768, (2, 400 * B)).astype(np.int16)
    hi, hq = golden["taps/FIR_SSB_I_coeffs"], golden["taps/FIR_SSB_Q_coeffs"]
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, 2, hi, hq, mixer=msdr.MIXER_NCO, mode=orclib.LSB, osc_i=oi, osc_q=oq)
    got = run_chain(ctx, chain, x, np.int16)
    assert chain.info()["time_segments"] > 1
    for c in range(2):
        assert np.array_equal(got[c], orc.chain_q15(x[c], orclib.LSB, hi, hq, mixer=1, osc_i=oi, osc_q=oq))


def test_chain_argument_errors(ctx, golden):
    hi = golden["taps/FIR_SSB_I_coeffs"]
    with pytest.raises(msdr.MsdrError) as e:
        msdr.Chain(ctx, msdr.ARITH_Q15, 1, hi[:85], hi[:85])               # odd numTaps (arm_fir_init_q15.c:93-96)
    assert e.value.status == msdr.STATUS_ARGUMENT_ERROR
    with pytest.raises(msdr.MsdrError):
        msdr.Chain(ctx, msdr.ARITH_F32, 1, hi.astype(np.float32), hi.astype(np.float32), mixer=msdr.MIXER_NCO)  # no tables
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, 1, hi, hi)
    chain.process(0, 0, 0)                                                  # empty block: no-op
    with pytest.raises(msdr.MsdrError):
        chain.process(0, 0, 128)                                            # null buffers


# ---------------------------------------------------------------- fp32 ---------------------
def _hilbert_pair(n_taps, fc=1330.0, fs=24000.0, bw=1920.0):
    """+-45 degree phase-added band-pass pair: Kaiser low-pass prototype modulated."""
    k = np.arange(n_taps)
    m = (n_taps - 1) / 2.0
    proto = np.sinc(2 * (bw / 2) / fs * (k - m)) * np.kaiser(n_taps, 6.0)
    proto /= proto.sum()
    w = 2 * np.pi * fc / fs
    hi = 2 * proto * np.cos(w * (k - m) + np.pi / 4)
    hq = 2 * proto * np.cos(w * (k - m) - np.pi / 4)
    return hi.astype(np.float32), hq.astype(np.float32)


def _f32_biquads(orc, stages):
    out = []
    for k, q in enumerate([0.54, 15.0, 0.54, 1.3][:stages]):
        kind = orclib.BQ_NOTCH if k == 1 else orclib.BQ_LOWPASS
        c = orc.biquad_design(kind, np.float32((3000 if k == 1 else 5400) * CORR), q).astype(np.float64) / 2 ** 30
        out.append([c[0], c[1], c[2], -c[3], -c[4]])
    return np.array(out, np.float32).reshape(-1, 5)


def _truth_f64(x, mode, hi, hq, oi, oq, bq, in_scale=1.0 / 32768):
    """The chain in float64 (same structure as orc_chain_f32, no rounding to speak of)."""
    x = x.astype(np.float64) * in_scale
    n = np.arange(x.size)
    i_s, q_s = x * oq.astype(np.float64)[n % oq.size], x * oi.astype(np.float64)[n % oi.size]
    i_f = np.convolve(i_s, hi.astype(np.float64)[::-1])[:x.size]
    q_f = np.convolve(q_s, hq.astype(np.float64)[::-1])[:x.size]
    d = i_f - q_f if mode == orclib.LSB else i_f + q_f if mode == orclib.USB else np.sqrt(i_f * i_f + q_f * q_f)
    if bq is not None:
        import scipy.signal
        for c in np.asarray(bq, np.float64).reshape(-1, 5):
            d = scipy.signal.lfilter(c[:3], [1.0, -c[3], -c[4]], d)
    return d


def _nco(p, cycles):
    n = np.arange(p)
    return np.sin(2 * np.pi * cycles * n / p).astype(np.float32), np.cos(2 * np.pi * cycles * n / p).astype(np.float32)


@pytest.mark.parametrize("ntaps,mode,stages,block", [
    (100, orclib.LSB, 2, None), (100, orclib.USB, 0, 128), (100, orclib.LSB, 2, 128),
    (61, orclib.AM, 4, None), (256, orclib.AM, 1, None), (512, orclib.CW, 2, 1000), (7, orclib.LSB, 1, 333)])
def test_chain_f32_nco_vs_oracle(ctx, orc, ntaps, mode, stages, block):
    rng = np.random.default_rng(ntaps + stages)
    hi, hq = _hilbert_pair(ntaps)
    oi, oq = _nco(128, 32)
    bq = _f32_biquads(orc, stages)
    x = rng.integers(-8000, 8001, (3, 6000)).astype(np.int16)
    x[1] = np.round(6000 * np.cos(2 * np.pi * 6700 * np.arange(6000) / 24000)).astype(np.int16)
    chain = msdr.Chain(ctx, msdr.ARITH_F32, 3, hi, hq, mixer=msdr.MIXER_NCO, mode=mode, osc_i=oi, osc_q=oq,
                       biquad_coeffs=bq if stages else None)
    got = run_chain(ctx, chain, x, np.float32, block)
    for c in range(3):
        want = orc.chain_f32(x[c], mode, hi, hq, oi, oq, bq if stages else None)
        err = rel_rms(got[c], want)
        if c == 1 and err >= TOL:
            # Channel 1 is a pure tone; where it falls on the SUPPRESSED sideband the output is what is left of a cancellation, ~50 dB
            # down, and a relative error of the output measures every evaluation's rounding against that remnant -- the sequential fp32
            # oracle's own included.  Judge both against a float64 evaluation of the same chain: the library must be no further from it
            # than the oracle is (it is closer: exact products, fp32 sums of 22-bit pieces).
            truth = _truth_f64(x[c], mode, hi, hq, oi, oq, bq if stages else None)
            assert rel_rms(got[c], truth) <= max(TOL, 1.5 * rel_rms(want, truth)), (c, err, rel_rms(got[c], truth), rel_rms(want, truth))
            continue
        assert err < TOL, (c, err)


@pytest.mark.parametrize("mode", [orclib.AM, orclib.LSB, orclib.USB])
def test_chain_f32_fs4_vs_oracle_and_q15(ctx, orc, golden, mode):
    """Fs/4 mixer in fp32 with the reference's own (Q15-scaled) tap sets: matches the fp32 oracle
    to 1e-5 and tracks the bit-exact q15 golden audio within the q15 truncation bound."""
    ti, tq = ("fir/taps_am102", "fir/taps_am102") if mode == orclib.AM else ("taps/FIR_SSB_I_coeffs", "taps/FIR_SSB_Q_coeffs")
    hi, hq = golden[ti].astype(np.float32) / 32768, golden[tq].astype(np.float32) / 32768
    sigs = ["am", "tones", "noise"]
    x = np.stack([golden["chain/x_" + s] for s in sigs])
    chain = msdr.Chain(ctx, msdr.ARITH_F32, 3, hi, hq, mixer=msdr.MIXER_FS4, mode=mode, in_scale=1.0)
    got = run_chain(ctx, chain, x, np.float32, 128)
    cos4, sin4 = np.array([1, 0, -1, 0], np.float32), np.array([0, 1, 0, -1], np.float32)
    mn = {orclib.AM: "AM", orclib.LSB: "LSB", orclib.USB: "USB"}[mode]
    for c, s in enumerate(sigs):
        want = orc.chain_f32(x[c], mode, hi, hq, sin4, cos4, None, in_scale=1.0)
        assert rel_rms(got[c], want) < TOL
        assert np.abs(got[c] - golden["chain/%s_%s_audio" % (s, mn)]).max() <= 3.0


def test_chain_f32_time_segments_vs_sequential(ctx, orc):
    """One channel, one long block: the GPU splits it into time segments and re-converges the IIR
    over a warm-up; result must stay within 1e-5 of the strictly sequential oracle, also right at
    the segment boundaries."""
    rng = np.random.default_rng(40)
    n = 1 << 20
    x = rng.integers(-8000, 8001, (1, n)).astype(np.int16)
    hi, hq = _hilbert_pair(100)
    oi, oq = _nco(128, 32)
    bq = _f32_biquads(orc, 2)                                   # LP + the Q=15 notch (slowest-decaying pole pair)
    chain = msdr.Chain(ctx, msdr.ARITH_F32, 1, hi, hq, mixer=msdr.MIXER_NCO, mode=orclib.LSB, osc_i=oi, osc_q=oq,
                       biquad_coeffs=bq)
    got = run_chain(ctx, chain, x, np.float32)
    info = chain.info()
    assert info["time_segments"] > 1 and info["warmup"] > 0
    want = orc.chain_f32(x[0], orclib.LSB, hi, hq, oi, oq, bq)
    assert rel_rms(got[0], want) < TOL
    seg = -(-n // info["time_segments"])
    seg = -(-seg // info["tile"]) * info["tile"]
    for s in range(1, info["time_segments"]):
        lo = s * seg
        if lo + 64 <= n:
            assert rel_rms(got[0, lo:lo + 64], want[lo:lo + 64]) < TOL, s
    # forcing exact state carry (time_segments=1) agrees as well, and so does a second call (state carried)
    chain1 = msdr.Chain(ctx, msdr.ARITH_F32, 1, hi, hq, mixer=msdr.MIXER_NCO, mode=orclib.LSB, osc_i=oi, osc_q=oq,
                        biquad_coeffs=bq, time_segments=1)
    got1 = run_chain(ctx, chain1, x[:, :200000], np.float32)
    assert chain1.info()["time_segments"] == 1
    assert rel_rms(got1[0], want[:200000]) < TOL


def test_chain_f32_mixed_modes_many_channels(ctx, orc):
    """C5 shape in small: per-channel AM/LSB select with per-mode tap sets, 512 taps, int16 in / fp32 out."""
    rng = np.random.default_rng(41)
    ch, n = 40, 5000
    lp = np.zeros(512, np.float32)
    lp[:] = (np.sinc(2 * 2800 / 24000 * (np.arange(512) - 255.5)) * np.kaiser(512, 7.0)).astype(np.float32)
    lp /= lp.sum()
    hi, hq = _hilbert_pair(512)
    modes = np.array([orclib.AM if (c * 2654435761) & 1 else orclib.LSB for c in range(ch)], np.int32)
    tapsets = np.array([0 if m == orclib.AM else 1 for m in modes], np.int32)
    x = rng.integers(-8000, 8001, (ch, n)).astype(np.int16)
    bq = _f32_biquads(orc, 1)
    chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, [lp, hi], [lp, hq], mixer=msdr.MIXER_FS4, modes=modes, tapsets=tapsets,
                       biquad_coeffs=bq)
    got = run_chain(ctx, chain, x, np.float32)
    cos4, sin4 = np.array([1, 0, -1, 0], np.float32), np.array([0, 1, 0, -1], np.float32)
    for c in range(ch):
        ti, tq = ([lp, hi][tapsets[c]], [lp, hq][tapsets[c]])
        want = orc.chain_f32(x[c], modes[c], ti, tq, sin4, cos4, bq)
        assert rel_rms(got[c], want) < TOL, c
    # retune one channel (msdr_chain_set_mode) and check it alone changes
    chain.reset()
    chain.set_mode(3, orclib.USB, 1)
    got2 = run_chain(ctx, chain, x, np.float32)
    want3 = orc.chain_f32(x[3], orclib.USB, hi, hq, sin4, cos4, bq)
    assert rel_rms(got2[3], want3) < TOL
    assert np.array_equal(got2[5], got[5])


# ---------------------------------------------------------------- fp32, folded kernel -------
def _q15_nco(p, cycles, length=128):
    """freq_conv-style tables: q15 oscillator tables (Osc_I/Q_buffer_i) converted like arm_q15_to_float;
    exactly periodic with period p samples."""
    n = np.arange(length)
    s = np.round(32767 * np.sin(2 * np.pi * cycles * n / p)).astype(np.int16)
    c = np.round(32767 * np.cos(2 * np.pi * cycles * n / p)).astype(np.int16)
    return (s / 32768.0).astype(np.float32), (c / 32768.0).astype(np.float32)


# folded FIR on the matrix cores (one wave per stream: the default) / on the fp32 VALU (the north-star's formulation)
ENGINES = {"mfw": 0, "valu": msdr.CHAIN_NO_MFMA}
ALL_ENGINES = ["mfw", "valu"]


def _mf_name(engine, stages, wg_waves=4):
    return "chain_mfw_kernel<%d>" % stages


@pytest.mark.parametrize("engine", ALL_ENGINES)
@pytest.mark.parametrize("period", [1, 2, 4])
@pytest.mark.parametrize("block", [None, 333, 128, 3073])
@pytest.mark.parametrize("mode", [orclib.LSB, orclib.USB])
def test_chain_f32_folded_ssb_vs_oracle(ctx, orc, period, block, mode, engine):
    """Short-period oscillators take a folded kernel (mixer folded into the taps): the split-fp16 matrix-core
    kernel, or with MSDR_CHAIN_NO_MFMA the packed-fp32 one.  Odd block lengths rotate the oscillator phase
    between calls and misalign the rows of channels > 0."""
    rng = np.random.default_rng(100 + period)
    hi, hq = _hilbert_pair(100)
    oi, oq = _q15_nco(period, 1)
    bq = _f32_biquads(orc, 2)
    x = rng.integers(-8000, 8001, (3, 7001)).astype(np.int16)
    chain = msdr.Chain(ctx, msdr.ARITH_F32, 3, hi, hq, mixer=msdr.MIXER_NCO, mode=mode, osc_i=oi, osc_q=oq, biquad_coeffs=bq,
                       flags=ENGINES[engine])
    got = run_chain(ctx, chain, x, np.float32, block)
    assert chain.info()["kernel"] == (_mf_name(engine, 2) if engine != "valu" else "chain_fold_kernel<%d>" % period)
    for c in range(3):
        want = orc.chain_f32(x[c], mode, hi, hq, oi, oq, bq)
        assert rel_rms(got[c], want) < TOL, (c, rel_rms(got[c], want))
    # the as-written kernel (MSDR_CHAIN_NO_TAP_FOLDING) agrees with the same oracle
    plain = msdr.Chain(ctx, msdr.ARITH_F32, 3, hi, hq, mixer=msdr.MIXER_NCO, mode=mode, osc_i=oi, osc_q=oq, biquad_coeffs=bq,
                       flags=msdr.CHAIN_NO_TAP_FOLDING)
    got2 = run_chain(ctx, plain, x, np.float32, block)
    assert plain.info()["kernel"] == "chain_kernel<ArithF32>"
    for c in range(3):
        assert rel_rms(got2[c], orc.chain_f32(x[c], mode, hi, hq, oi, oq, bq)) < TOL


@pytest.mark.parametrize("engine", ALL_ENGINES)
@pytest.mark.parametrize("block", [None, 129, 1000])
def test_chain_f32_folded_am_fs4_odd_blocks(ctx, orc, block, engine):
    """AM through the folded kernel (Fs/4 zero skipping) with block lengths that leave the mixer at
    every phase 0..3 at a call boundary."""
    rng = np.random.default_rng(77)
    lp = (np.sinc(2 * 2800 / 24000 * (np.arange(62) - 30.5)) * np.kaiser(62, 7.0)).astype(np.float32)
    lp /= lp.sum()
    x = rng.integers(-8000, 8001, (2, 5003)).astype(np.int16)
    bq = _f32_biquads(orc, 1)
    chain = msdr.Chain(ctx, msdr.ARITH_F32, 2, lp, lp, mixer=msdr.MIXER_FS4, mode=orclib.AM, biquad_coeffs=bq, flags=ENGINES[engine])
    got = run_chain(ctx, chain, x, np.float32, block)
    assert chain.info()["kernel"] == (_mf_name(engine, len(bq)) if engine != "valu" else "chain_fold_kernel<4>")
    cos4, sin4 = np.array([1, 0, -1, 0], np.float32), np.array([0, 1, 0, -1], np.float32)
    for c in range(2):
        assert rel_rms(got[c], orc.chain_f32(x[c], orclib.AM, lp, lp, sin4, cos4, bq)) < TOL


def _lowpass(ntaps, seed=0):
    k = np.arange(ntaps) - (ntaps - 1) / 2
    lp = (np.sinc(2 * (2800 + 100 * seed) / 24000 * k) * np.kaiser(ntaps, 7.0)).astype(np.float32)
    return (lp / lp.sum()).astype(np.float32)


@pytest.mark.parametrize("stages", [0, 1, 2, 4])
@pytest.mark.parametrize("ntaps", [2, 33, 62, 129, 200, 256, 257])
def test_chain_f32_envelope_taps_in_registers(ctx, orc, ntaps, stages, monkeypatch):
    """chain_amtr_kernel (envelope channels, both FIRs the same taps, exact Fs/4 mixer): every step count (2..257 taps) and cascade
    length, two tap sets, blocks that end inside a tile / at every mixer phase, state carried between the calls.  By default the host
    picks this kernel only where it measured faster (256-tap class, <= 1 section): MSDR_AMTR=1 makes it take every eligible chain."""
    monkeypatch.setenv("MSDR_AMTR", "1")
    rng = np.random.default_rng(500 + ntaps + stages)
    lps = [_lowpass(ntaps, 0), _lowpass(ntaps, 3)]
    bq = _f32_biquads(orc, stages)
    x = rng.integers(-12000, 12001, (3, 9001)).astype(np.int16)
    tapsets = [0, 1, 0]
    cos4, sin4 = np.array([1, 0, -1, 0], np.float32), np.array([0, 1, 0, -1], np.float32)
    want = [orc.chain_f32(x[c], orclib.AM, lps[tapsets[c]], lps[tapsets[c]], sin4, cos4, bq) for c in range(3)]
    for block in (None, 3073, 1000, 129):
        chain = msdr.Chain(ctx, msdr.ARITH_F32, 3, lps, lps, mixer=msdr.MIXER_FS4, mode=orclib.AM, tapsets=tapsets, biquad_coeffs=bq)
        got = run_chain(ctx, chain, x, np.float32, block)
        assert chain.info()["kernel"] == "chain_amtr_kernel"
        for c in range(3):
            assert rel_rms(got[c], want[c]) < TOL, (block, c, rel_rms(got[c], want[c]))


def test_chain_f32_envelope_taps_in_registers_default_rule_and_mixed_modes(ctx, orc, monkeypatch):
    """Without MSDR_AMTR the host takes the kernel for the 256-tap class with at most one section only; SSB channels of the same chain
    stay on the wave-stream kernel (two launches), and a long block is cut into time segments with a settled cascade."""
    monkeypatch.delenv("MSDR_AMTR", raising=False)
    rng = np.random.default_rng(41)
    lp = _lowpass(256)
    cos4, sin4 = np.array([1, 0, -1, 0], np.float32), np.array([0, 1, 0, -1], np.float32)
    for stages, name in ((1, "chain_mfw_kernel + chain_amtr_kernel"), (2, "chain_mfw_kernel<2>")):
        bq = _f32_biquads(orc, stages)
        modes = [orclib.AM, orclib.LSB, orclib.AM, orclib.USB]
        x = rng.integers(-12000, 12001, (4, 6000)).astype(np.int16)
        chain = msdr.Chain(ctx, msdr.ARITH_F32, 4, lp, lp, mixer=msdr.MIXER_FS4, modes=modes, biquad_coeffs=bq)
        got = run_chain(ctx, chain, x, np.float32, 2500)
        assert chain.info()["kernel"] == name
        for c in range(4):
            assert rel_rms(got[c], orc.chain_f32(x[c], modes[c], lp, lp, sin4, cos4, bq)) < TOL, (stages, c)
    n = 1 << 19
    x = rng.integers(-12000, 12001, (1, n)).astype(np.int16)
    bq = _f32_biquads(orc, 1)
    chain = msdr.Chain(ctx, msdr.ARITH_F32, 1, lp, lp, mixer=msdr.MIXER_FS4, mode=orclib.AM, biquad_coeffs=bq)
    got = run_chain(ctx, chain, x, np.float32)
    info = chain.info()
    assert info["kernel"] == "chain_amtr_kernel" and info["time_segments"] > 1
    want = orc.chain_f32(x[0], orclib.AM, lp, lp, sin4, cos4, bq)
    assert rel_rms(got[0], want) < TOL
    seg = -(-n // info["time_segments"])
    seg = -(-seg // info["tile"]) * info["tile"]
    for sgi in range(1, info["time_segments"]):
        lo = sgi * seg
        if lo + 64 <= n:
            assert rel_rms(got[0, lo:lo + 64], want[lo:lo + 64]) < TOL, sgi


def test_wave_stream_workgroup_is_whole_waves_per_simd(ctx, orc, monkeypatch):
    """msdr_chain_create sizes the wave-stream kernel's workgroup in whole waves per SIMD: the 40 KB of fragments of a 256-tap envelope
    table leave LDS for 13 - 16 windows, and 13 waves (4 + 3 + 3 + 3 over the SIMDs) ran 4 % behind 12 per tile (profiles/r03/c3_trims.txt)."""
    monkeypatch.delenv("MSDR_AMTR", raising=False)
    rng = np.random.default_rng(321)
    lp = _lowpass(256)
    cos4, sin4 = np.array([1, 0, -1, 0], np.float32), np.array([0, 1, 0, -1], np.float32)
    bq = _f32_biquads(orc, 2)
    x = rng.integers(-12000, 12001, (8, 5000)).astype(np.int16)
    chain = msdr.Chain(ctx, msdr.ARITH_F32, 8, lp, lp, mixer=msdr.MIXER_FS4, mode=orclib.AM, biquad_coeffs=bq)
    got = run_chain(ctx, chain, x, np.float32, 2048)
    info = chain.info()
    assert info["kernel"] == "chain_mfw_kernel<2>"
    waves = info["block"] // 64
    on_cu = min(16 // waves, (160 * 1024) // info["lds_bytes"]) * waves
    assert on_cu >= 8 and on_cu % 4 == 0, info
    for c in (0, 7):
        assert rel_rms(got[c], orc.chain_f32(x[c], orclib.AM, lp, lp, sin4, cos4, bq)) < TOL


@pytest.mark.parametrize("engine", ALL_ENGINES)
def test_chain_f32_am_with_non_fs4_nco(ctx, orc, engine):
    """The packed-fp32 folded kernel does AM only for the exact Fs/4 pattern: a q15-rounded fs/4 table (0.99997)
    falls back to the as-written kernel there.  The matrix-core kernel takes any short-period table."""
    rng = np.random.default_rng(78)
    hi, hq = _hilbert_pair(100)
    oi, oq = _q15_nco(4, 1)
    x = rng.integers(-8000, 8001, (2, 4000)).astype(np.int16)
    chain = msdr.Chain(ctx, msdr.ARITH_F32, 2, hi, hq, mixer=msdr.MIXER_NCO, modes=np.array([orclib.AM, orclib.LSB], np.int32),
                       osc_i=oi, osc_q=oq, flags=ENGINES[engine])
    got = run_chain(ctx, chain, x, np.float32)
    assert chain.info()["kernel"] == (_mf_name(engine, 0) if engine != "valu" else "chain_kernel<ArithF32>")
    for c, m in enumerate((orclib.AM, orclib.LSB)):
        assert rel_rms(got[c], orc.chain_f32(x[c], m, hi, hq, oi, oq, None)) < TOL


# ---------------------------------------------------------------- fp32, long FIRs behind a general oscillator table ---
def _general_table_case(ntaps, mode):
    if mode == orclib.AM:
        hi = (np.sinc(2 * 2800 / 24000 * (np.arange(ntaps) - (ntaps - 1) / 2)) * np.kaiser(ntaps, 7.0)).astype(np.float32)
        hi /= hi.sum()
        hq = hi
    else:
        hi, hq = _hilbert_pair(ntaps)
    return hi, hq


@pytest.mark.parametrize("ntaps", [130, 248, 257, 513, 1021])
@pytest.mark.parametrize("mode", [orclib.LSB, orclib.USB, orclib.AM])
def test_chain_f32_long_fir_behind_a_general_table_vs_oracle(ctx, orc, ntaps, mode):
    """Long filters behind an oscillator table that is NOT short-periodic (every AudioEffectFreqConv table repeats with the 128-sample block
    whatever is in it, freq_conv.cpp:67-103).  Round 4 stopped at 247 taps and fell to the vector ALU (256 taps 0.07, 512 taps 0.04 of the roof
    on c4's shape).  Round 5: from 128 taps on the full-rate layout keeps the B operand as shifted copies of the taps (mw_compact_stride: 19 KB
    per filter at 512 taps where the k-step fragments are 68 KB), so every length to 1021+ taps stays on the matrix cores: 256 taps 0.18, 512
    taps 0.098 = 0.90 PFLOP/s executed (profiles/r05/nco_long_taps.txt)."""
    rng = np.random.default_rng(ntaps * 3 + mode)
    hi, hq = _general_table_case(ntaps, mode)
    oi, oq = _nco(128, 5)                                   # 5 cycles per 128 samples: period 128
    bq = _f32_biquads(orc, 2)
    x = rng.integers(-8000, 8001, (3, 20011)).astype(np.int16)
    chain = msdr.Chain(ctx, msdr.ARITH_F32, 3, hi, hq, mixer=msdr.MIXER_NCO, mode=mode, osc_i=oi, osc_q=oq, biquad_coeffs=bq)
    for block in (None, 4999, 128):
        chain.reset()
        got = run_chain(ctx, chain, x, np.float32, block)
        if block != 128:
            assert chain.info()["kernel"] == "chain_mfw_kernel<2> full-rate NCO streams", chain.info()
        for c in range(3):
            want = orc.chain_f32(x[c], mode, hi, hq, oi, oq, bq)
            assert rel_rms(got[c], want) < TOL, (block, c, rel_rms(got[c], want))


@pytest.mark.parametrize("stages", [0, 1, 2, 4])
@pytest.mark.parametrize("ntaps", [57, 100, 248, 330])
def test_chain_f32_full_rate_layouts_agree(ctx, orc, monkeypatch, ntaps, stages):
    """The two B-operand layouts of the full-rate kernel (k-step fragments, MSDR_FR_COMPACT=0; shifted copies of the taps, =1) on the same
    chains, every flavour (LSB / USB / envelope with two different low-passes / envelope with one) and section count: both inside the
    tolerance against the oracle.  (With 1 - 2 sections the fragment layout folds the cascade into its SSB columns, the compact one runs it
    as the lane scan: the two differ by rounding there, elsewhere they run the same products in the same order -- bit-identical.)"""
    rng = np.random.default_rng(ntaps * 7 + stages)
    oi, oq = _nco(128, 9)
    bq = _f32_biquads(orc, stages) if stages else None
    x = rng.integers(-8000, 8001, (4, 9000)).astype(np.int16)
    modes = np.array([orclib.LSB, orclib.USB, orclib.AM, orclib.CW], np.int32)
    hi, hq = _hilbert_pair(ntaps)
    lp, _ = _general_table_case(ntaps, orclib.AM)
    for ti, tq in ((hi, hq), (lp, lp)):
        outs = []
        for layout in ("0", "1"):
            monkeypatch.setenv("MSDR_FR_COMPACT", layout)
            chain = msdr.Chain(ctx, msdr.ARITH_F32, 4, ti, tq, mixer=msdr.MIXER_NCO, modes=modes, osc_i=oi, osc_q=oq, biquad_coeffs=bq)
            outs.append(run_chain(ctx, chain, x, np.float32, 3001))
            assert chain.info()["kernel"].endswith("full-rate NCO streams"), chain.info()
        monkeypatch.delenv("MSDR_FR_COMPACT")
        for c in range(4):
            want = orc.chain_f32(x[c], modes[c], ti, tq, oi, oq, bq)
            for o in outs:
                assert rel_rms(o[c], want) < TOL, (ntaps, stages, c, rel_rms(o[c], want))
            if stages in (0, 4) or modes[c] in (orclib.AM, orclib.CW):
                assert np.array_equal(outs[0][c].view(np.uint32), outs[1][c].view(np.uint32)), (ntaps, stages, c)


def test_chain_f32_valu_envelope_with_distinct_branches(ctx, orc):
    rng = np.random.default_rng(5)
    hi, hq = _hilbert_pair(256)
    x = rng.integers(-8000, 8001, (2, 6000)).astype(np.int16)
    chain = msdr.Chain(ctx, msdr.ARITH_F32, 2, hi, hq, mixer=msdr.MIXER_FS4, mode=orclib.CW, flags=msdr.CHAIN_NO_MFMA)
    got = run_chain(ctx, chain, x, np.float32)
    assert chain.info()["kernel"] == "chain_fold_kernel<4>"
    cos4, sin4 = np.array([1, 0, -1, 0], np.float32), np.array([0, 1, 0, -1], np.float32)
    for c in range(2):
        assert rel_rms(got[c], orc.chain_f32(x[c], orclib.CW, hi, hq, sin4, cos4, None)) < TOL


@pytest.mark.parametrize("engine", ALL_ENGINES)
def test_chain_f32_time_segments_long_stream(ctx, orc, engine):
    rng = np.random.default_rng(6)
    n = 1 << 20
    x = rng.integers(-8000, 8001, (1, n)).astype(np.int16)
    hi, hq = _hilbert_pair(256)
    oi, oq = _q15_nco(4, 1)
    bq = _f32_biquads(orc, 2)
    chain = msdr.Chain(ctx, msdr.ARITH_F32, 1, hi, hq, mixer=msdr.MIXER_NCO, mode=orclib.LSB, osc_i=oi, osc_q=oq, biquad_coeffs=bq,
                       flags=ENGINES[engine])
    got = run_chain(ctx, chain, x, np.float32)
    info = chain.info()
    assert info["kernel"] == (_mf_name(engine, 2, 8) if engine != "valu" else "chain_fold_kernel<4>") and info["time_segments"] > 1
    want = orc.chain_f32(x[0], orclib.LSB, hi, hq, oi, oq, bq)
    assert rel_rms(got[0], want) < TOL


# ---------------------------------------------------------------- fp32, matrix-core kernel ---------
@pytest.mark.parametrize("ntaps", [1, 2, 31, 33, 64, 100, 129, 256, 512])
@pytest.mark.parametrize("mode", [orclib.LSB, orclib.AM])
@pytest.mark.parametrize("engine", ["mfw"])
def test_chain_f32_mfma_tap_counts(ctx, orc, ntaps, mode, engine):
    """The Toeplitz operand is built per tap count (halo = ntaps - 1 rounded up to 32); Fs/4 mixer, mixed block sizes,
    three channels so that rows of channels > 0 are misaligned for odd n."""
    rng = np.random.default_rng(900 + ntaps)
    if ntaps < 8:
        hi = rng.standard_normal(ntaps).astype(np.float32)
        hq = rng.standard_normal(ntaps).astype(np.float32)
    else:
        hi, hq = _hilbert_pair(ntaps)
    bq = _f32_biquads(orc, 2)
    cos4, sin4 = np.array([1, 0, -1, 0], np.float32), np.array([0, 1, 0, -1], np.float32)
    for n in (12288 + 8, 9001):
        x = rng.integers(-32768, 32768, (3, n)).astype(np.int16)
        chain = msdr.Chain(ctx, msdr.ARITH_F32, 3, hi, hq, mixer=msdr.MIXER_FS4, mode=mode, biquad_coeffs=bq, flags=ENGINES[engine])
        for block in (None, 4100):
            chain.reset()
            got = run_chain(ctx, chain, x, np.float32, block)
            assert chain.info()["kernel"] == _mf_name(engine, 2, 4 if ntaps <= 129 else 8), chain.info()
            for c in range(3):
                want = orc.chain_f32(x[c], mode, hi, hq, sin4, cos4, bq)
                assert rel_rms(got[c], want) < TOL, (n, block, c, rel_rms(got[c], want))


@pytest.mark.parametrize("engine", ["mfw"])
def test_chain_f32_mfma_weak_signal_keeps_fp32_accuracy(ctx, orc, engine):
    """The fp16 split of the samples is a FLOATING split (11 significant bits + exact remainder), so a weak signal
    (|x| <= 40) is as accurate as a full-scale one; full-scale extremes (-32768, 32767) are exact too."""
    rng = np.random.default_rng(31)
    hi, hq = _hilbert_pair(100)
    cos4, sin4 = np.array([1, 0, -1, 0], np.float32), np.array([0, 1, 0, -1], np.float32)
    weak = rng.integers(-40, 41, (1, 8192)).astype(np.int16)
    rail = rng.choice(np.array([-32768, 32767, -32767, 32766, 2049, -2049], np.int16), (1, 8192))
    for x in (weak, rail):
        chain = msdr.Chain(ctx, msdr.ARITH_F32, 1, hi, hq, mixer=msdr.MIXER_FS4, mode=orclib.USB, flags=ENGINES[engine])
        got = run_chain(ctx, chain, x, np.float32)
        assert chain.info()["kernel"] == _mf_name(engine, 0)
        assert rel_rms(got[0], orc.chain_f32(x[0], orclib.USB, hi, hq, sin4, cos4, None)) < 2e-6


@pytest.mark.parametrize("engine", ALL_ENGINES)
def test_chain_f32_retune_mid_stream_keeps_cascade_state(ctx, orc, engine):
    """msdr_chain_set_mode between calls: FIR history and biquad state carry over, as in the oracle with a carried state.
    The matrix-core kernel's SSB modes fold the cascade's numerator into the FIR; entering / leaving / changing such a mode
    must not show (numerator history rebuilt, resp. a correction to the first samples)."""
    rng = np.random.default_rng(55)
    hi, hq = _hilbert_pair(100)
    bq = _f32_biquads(orc, 2)
    cos4, sin4 = np.array([1, 0, -1, 0], np.float32), np.array([0, 1, 0, -1], np.float32)
    x = rng.integers(-8000, 8001, (2, 6 * 1500)).astype(np.int16)
    plan = [orclib.LSB, orclib.AM, orclib.USB, orclib.LSB, orclib.CW, orclib.USB]     # channel 0; channel 1 stays LSB
    chain = msdr.Chain(ctx, msdr.ARITH_F32, 2, hi, hq, mixer=msdr.MIXER_FS4, mode=orclib.LSB, biquad_coeffs=bq, flags=ENGINES[engine])
    st0, st1 = {}, {}
    for k, m in enumerate(plan):
        if k:
            chain.set_mode(0, m, 0)
            if k == 3:                       # retuned twice before the next sample
                chain.set_mode(0, orclib.AM, 0)
                chain.set_mode(0, m, 0)
        seg = x[:, 1500 * k:1500 * (k + 1)]
        got = run_chain(ctx, chain, seg, np.float32)
        want0 = orc.chain_f32(seg[0], m, hi, hq, sin4, cos4, bq, state=st0)
        want1 = orc.chain_f32(seg[1], orclib.LSB, hi, hq, sin4, cos4, bq, state=st1)
        assert rel_rms(got[0], want0) < TOL, (k, m, rel_rms(got[0], want0))
        assert rel_rms(got[1], want1) < TOL, (k, rel_rms(got[1], want1))


@pytest.mark.parametrize("stages", [1, 2])
@pytest.mark.parametrize("ntaps", [3, 40])
def test_chain_f32_retune_between_tap_sets_of_very_different_gain(ctx, orc, stages, ntaps):
    """The cascade's state and numerator history that one (mode, tap set) leaves behind enter the next one's kernel through
    fp16 at the NEW table's scale.  A loud tap set followed by one with 1/50 of its gain used to saturate there (first rows
    after the switch wrong by 2-30 %; found by tests/debug/fuzz_retune.py): the table scales are bounded chain-wide now."""
    rng = np.random.default_rng(77)
    loud_i = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
    loud_q = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
    quiet = (0.02 * rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
    sets_i, sets_q = [quiet, loud_i], [quiet.copy(), loud_q]
    bq = _f32_biquads(orc, stages)
    cos4, sin4 = np.array([1, 0, -1, 0], np.float32), np.array([0, 1, 0, -1], np.float32)
    plan = [(orclib.CW, 1), (orclib.AM, 0), (orclib.USB, 1), (orclib.LSB, 0), (orclib.AM, 1), (orclib.CW, 0), (orclib.LSB, 1), (orclib.AM, 0)]
    x = rng.integers(-20000, 20001, (2, 1408 * len(plan))).astype(np.int16)
    chain = msdr.Chain(ctx, msdr.ARITH_F32, 2, sets_i, sets_q, mixer=msdr.MIXER_FS4, modes=np.array([plan[0][0], orclib.LSB], np.int32),
                       tapsets=np.array([plan[0][1], 1], np.int32), biquad_coeffs=bq)
    st0, st1 = {}, {}
    for k, (m, ts) in enumerate(plan):
        if k:
            chain.set_mode(0, m, ts)
        seg = x[:, 1408 * k:1408 * (k + 1)]
        got = run_chain(ctx, chain, seg, np.float32)
        assert chain.info()["kernel"].startswith("chain_mfw_kernel")
        want0 = orc.chain_f32(seg[0], m, sets_i[ts], sets_q[ts], sin4, cos4, bq, state=st0)
        want1 = orc.chain_f32(seg[1], orclib.LSB, sets_i[1], sets_q[1], sin4, cos4, bq, state=st1)
        assert rel_rms(got[0], want0) < TOL, (k, m, ts, rel_rms(got[0], want0))
        assert rel_rms(got[1], want1) < TOL, (k, rel_rms(got[1], want1))


def test_chain_f32_mfw_repeatable_long_stream(ctx, orc):
    """Many short segments, a long halo (256 taps) and the folded IIR: every launch must give the same, correct stream.  (A
    variant of the kernel that took the scan's uniform matrices through the scalar cache gave intermittently wrong rows
    in exactly this configuration; eight fresh chains in a row catch that kind of fault.)"""
    rng = np.random.default_rng(6)
    n = 1 << 20
    x = rng.integers(-8000, 8001, (1, n)).astype(np.int16)
    hi, hq = _hilbert_pair(256)
    oi, oq = _q15_nco(4, 1)
    bq = _f32_biquads(orc, 2)
    want = orc.chain_f32(x[0], orclib.LSB, hi, hq, oi, oq, bq)
    first = None
    for rep in range(8):
        chain = msdr.Chain(ctx, msdr.ARITH_F32, 1, hi, hq, mixer=msdr.MIXER_NCO, mode=orclib.LSB, osc_i=oi, osc_q=oq, biquad_coeffs=bq)
        got = run_chain(ctx, chain, x, np.float32)[0]
        assert rel_rms(got, want) < TOL, rep
        if first is None:
            first = got
        assert np.array_equal(got, first), rep          # bit-identical from launch to launch


# ---------------------------------------------------------------- q15 on the integer matrix cores ----
QM, VALU = "chain_q15mf_kernel", "chain_kernel<ArithQ15>"


@pytest.mark.parametrize("mn,mode,ti,tq", CHAIN)
@pytest.mark.parametrize("flags,kernel", [(0, QM), (msdr.CHAIN_NO_MFMA, VALU)])
def test_chain_q15_both_kernels_match_reference_golden(ctx, golden, mn, mode, ti, tq, flags, kernel, monkeypatch):
    """The matrix-core kernel (default with the Fs/4 mixer) and the VALU kernel against the reference-generated vectors.
    (MSDR_NO_BLOCK=1: 128-sample calls through the STREAMING kernel's cold tiles; the block kernel's turn is tests/test_gpu_block.py.)"""
    monkeypatch.setenv("MSDR_NO_BLOCK", "1")
    sigs = ["am", "tones", "noise", "full"]
    x = np.stack([golden["chain/x_" + s] for s in sigs])
    for sk, suffix in ((msdr.SQRT_F32, ""), (msdr.SQRT_Q31, "_q31")):
        if suffix and mn not in ("AM", "CW"):
            continue
        chain = msdr.Chain(ctx, msdr.ARITH_Q15, len(sigs), golden[ti], golden[tq], mode=mode, sqrt_kind=sk, flags=flags)
        got = run_chain(ctx, chain, x, np.int16, 128)
        assert chain.info()["kernel"] == kernel
        for c, s in enumerate(sigs):
            assert np.array_equal(got[c], golden["chain/%s_%s_audio%s" % (s, mn, suffix)]), (s, mn, kernel)


@pytest.mark.parametrize("ntaps", [2, 30, 62, 100, 256, 512])
def test_chain_q15_matrix_core_tap_counts_and_ragged_blocks(ctx, orc, ntaps):
    """Any even tap count up to 512, blocks of ragged lengths (the mixer phase of a call's first sample cycles through
    0..3, rows lose their 16-byte alignment, tiles are partial), full-scale input with -32768 runs."""
    rng = np.random.default_rng(ntaps)
    ch, n = 5, 19 * B
    x = rng.integers(-32768, 32768, (ch, n)).astype(np.int16)
    x[0, ::3] = -32768
    x[1, :] = -32768
    x[2, ::2] = 32767
    ci = rng.integers(-3000, 3001, ntaps).astype(np.int16)
    cq = rng.integers(-3000, 3001, ntaps).astype(np.int16)
    modes = np.array([orclib.AM, orclib.LSB, orclib.USB, orclib.CW, orclib.SYNCAM], np.int32)
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, ci, cq, modes=modes)
    got = np.empty_like(x)
    o = 0
    for m in [130, 7, 1025, 1, 2, 129, 3] + [n]:                 # the last entry takes the rest
        m = min(m, n - o)
        dx, dy = ctx.to_device(x[:, o:o + m]), ctx.array((ch, m), np.int16)
        chain.process(dx, dy, m)
        got[:, o:o + m] = dy.download()
        assert chain.info()["kernel"] == QM
        o += m
        if o >= n:
            break
    for c in range(ch):
        assert np.array_equal(got[c], orc.chain_q15(x[c], modes[c], ci, cq)), (ntaps, c)


def test_chain_q15_matrix_core_accumulator_wraps_and_large_taps_fall_back(ctx, orc):
    """arm_fir_fast_q15's 32-bit accumulator wraps (arm_fir_fast_q15.c:49-53): taps of 32639 x full-scale input force it.
    A tap >= 32640 does not split into two signed bytes: that tap set runs on the VALU kernel -- same results."""
    rng = np.random.default_rng(77)
    x = rng.integers(-32768, 32768, (3, 12 * B)).astype(np.int16)
    x[1] = np.where(np.arange(12 * B) % 4 < 2, 32767, -32768)     # after the Fs/4 signs every product has the same sign
    for big, kernel in ((32639, QM), (32767, VALU), (-32768, QM)):
        taps = np.full(64, big, np.int16)
        for mode in (orclib.LSB, orclib.AM):
            chain = msdr.Chain(ctx, msdr.ARITH_Q15, 3, taps, taps, mode=mode)
            got = run_chain(ctx, chain, x, np.int16, None)
            assert chain.info()["kernel"] == kernel
            for c in range(3):
                want, i_f, q_f = orc.chain_q15(x[c], mode, taps, taps, want_iq=True)
                assert np.array_equal(got[c], want), (big, mode, c)
            if big == 32639 and mode == orclib.LSB:
                assert (np.abs(i_f.astype(np.int32)) == 32768).any() or (i_f == 32767).any()      # the FIR output saturates somewhere


def test_chain_q15_matrix_core_time_segments_and_tapsets(ctx, orc, golden):
    """Long blocks are cut into time segments (exact for a FIR: no state but the sample history); channels with different
    tap sets and demodulators are separate launches."""
    rng = np.random.default_rng(5)
    ch, n = 7, 96 * B
    x = rng.integers(-20000, 20001, (ch, n)).astype(np.int16)
    sets_i = [golden["fir/taps_lp256"], np.concatenate([np.zeros(256 - 86, np.int16), golden["taps/FIR_SSB_I_coeffs"]])]
    sets_q = [golden["fir/taps_lp256"], np.concatenate([np.zeros(256 - 86, np.int16), golden["taps/FIR_SSB_Q_coeffs"]])]
    modes = np.array([orclib.AM, orclib.LSB, orclib.USB, orclib.AM, orclib.LSB, orclib.CW, orclib.USB], np.int32)
    tapsets = np.array([0, 1, 1, 0, 1, 0, 1], np.int32)
    for seg in (0, 3, 12):
        chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, sets_i, sets_q, modes=modes, tapsets=tapsets, time_segments=seg)
        got = run_chain(ctx, chain, x, np.int16, None)
        info = chain.info()
        assert info["kernel"] == QM
        for c in range(ch):
            assert np.array_equal(got[c], orc.chain_q15(x[c], modes[c], sets_i[tapsets[c]], sets_q[tapsets[c]])), (seg, c)
    # a mode change regroups the channels
    chain.set_mode(0, orclib.USB, 1)
    got = run_chain(ctx, chain, x, np.int16, None)       # (the history carries over: compare the tail, past the FIR's memory)
    want = orc.chain_q15(x[0], orclib.USB, sets_i[1], sets_q[1])
    assert np.array_equal(got[0][512:], want[512:])


@pytest.mark.parametrize("mixer", [0, 1])
def test_chain_q15_retune_mid_stream_is_bit_exact(ctx, orc, golden, mixer, monkeypatch):
    """msdr_chain_set_mode between calls on the Q15 chain: the FIR history (raw IF samples, mixed again at staging) and the two
    biquad nodes' state carry over, the channel groups per (tap set, demodulator) are rebuilt -- bit-exact against the oracle
    run with a carried state.  (tests/debug/fuzz_retune_q15.py is the randomised version: 56 000 plans, 0 mismatches.)"""
    monkeypatch.setenv("MSDR_NO_BLOCK", "1")        # (one of the calls is a single block: the streaming kernel's turn here, tests/test_gpu_block.py has the block kernel's)
    rng = np.random.default_rng(90 + mixer)
    ch = 70
    pad = lambda t: np.concatenate([np.zeros(102 - t.size, np.int16), t])
    sets_i = [golden["fir/taps_am102"], pad(golden["taps/FIR_SSB_I_coeffs"]), pad(golden["taps/FIR_CW_I_coeffs"])]
    sets_q = [golden["fir/taps_am102"], pad(golden["taps/FIR_SSB_Q_coeffs"]), pad(golden["taps/FIR_CW_Q_coeffs"])]
    lp, nt = _ref_nodes(orc)
    oi = oq = None
    if mixer:
        k = np.arange(B)
        oi = np.round(32767 * np.sin(2 * np.pi * k / 4)).astype(np.int16)
        oq = np.round(32767 * np.cos(2 * np.pi * k / 4)).astype(np.int16)
    modes = rng.integers(1, 5, ch).astype(np.int32)
    tapsets = rng.integers(0, 3, ch).astype(np.int32)
    lens = [5 * B, B, 9 * B, 3 * B, 6 * B]
    x = rng.integers(-20000, 20001, (ch, sum(lens))).astype(np.int16)
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, sets_i, sets_q, mixer=mixer, modes=modes, tapsets=tapsets, osc_i=oi, osc_q=oq,
                       biquad_nodes=[[lp], [nt]])
    watch = [0, 1, 17, 63, 64, 69]
    states = {c: {} for c in watch}
    o = 0
    for j, m in enumerate(lens):
        if j:
            for c in watch[j % 2::2] + [5, 40]:                      # half of the watched channels, and two unwatched ones
                modes[c], tapsets[c] = int(rng.integers(1, 5)), int(rng.integers(0, 3))
                chain.set_mode(c, int(modes[c]), int(tapsets[c]))
        seg = np.ascontiguousarray(x[:, o:o + m])
        got = run_chain(ctx, chain, seg, np.int16)
        assert chain.info()["kernel"].startswith(QM)
        for c in watch:
            want = orc.chain_q15(seg[c], int(modes[c]), sets_i[tapsets[c]], sets_q[tapsets[c]], mixer=mixer, osc_i=oi, osc_q=oq,
                                 biquads=[orc.biquad_teensy_new([lp]), orc.biquad_teensy_new([nt])], state=states[c])
            assert np.array_equal(got[c], want), (j, c, int(modes[c]), int(tapsets[c]))
        o += m


@pytest.mark.parametrize("ch", [64, 192])
def test_chain_q15_two_biquad_nodes_pipeline(ctx, orc, golden, ch):
    """biquad1_dac -> biquad2_dac on whole 64-channel groups runs as a two-wave pipeline (one node per wave): multi-stage nodes,
    state carried over calls, inputs that drive the Teensy biquad into saturation."""
    rng = np.random.default_rng(ch)
    n = 10 * B
    x = rng.integers(-32768, 32768, (ch, n)).astype(np.int16)
    x[1] = np.where((np.arange(n) // 40) % 2, 32767, -32768)                     # square wave at full scale
    taps = golden["fir/taps_am102"]
    corr = CORR
    lr = [orc.biquad_design(orclib.BQ_LOWPASS, np.float32(5400 * corr), q) for q in (0.54, 1.3, 0.54, 1.3)]     # .ino:393-399
    nt = orc.biquad_design(orclib.BQ_NOTCH, np.float32(3000 * corr), 15.0)
    hs = orc.biquad_design(orclib.BQ_HIGHSHELF, np.float32(2000.0), 9.0, 0.8)
    for nodes in ([lr, [nt]], [[nt], [hs, nt]]):
        chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, taps, taps, mode=orclib.LSB, biquad_nodes=nodes)
        got = run_chain(ctx, chain, x, np.int16, 2 * B, node_kernel="biquad_teensy_pipe_kernel")      # five calls of two slabs each
        for c in list(range(0, ch, 13)) + [1, ch - 1]:
            want = orc.chain_q15(x[c], orclib.LSB, taps, taps, biquads=[orc.biquad_teensy_new(nd) for nd in nodes])
            assert np.array_equal(got[c], want), (ch, c)


@pytest.mark.parametrize("per_group", [16, 32, 64])
@pytest.mark.parametrize("block", [B, 2 * B, 3 * B, None])
def test_chain_q15_one_stage_nodes_on_the_slab_pipeline(ctx, orc, golden, block, per_group, monkeypatch):
    """The reference's configuration -- one stage per node (low-pass .ino:391-393, Q = 15 notch .ino:356) -- on whole 64-channel groups:
    biquad_teensy_pipe4_kernel<2, per_group> (the two recursions alone on two waves) for calls of two and three slabs (the pipeline's
    start-up and drain paths) and one long call.  Calls of ONE slab are the block cadence: there the nodes run as the second phase of
    chain_q15mb_kernel, whatever per_group says (the node kernels at that length: tests/test_gpu_q15_ladders.py, tests/test_gpu_block.py).
    Full-scale square wave; state carried from call to call."""
    monkeypatch.setenv("MSDR_BIQUAD_PIPE_CH", str(per_group))      # channels per workgroup (read when the nodes are created)
    rng = np.random.default_rng(7)
    ch, n = 128, 12 * B
    x = rng.integers(-32768, 32768, (ch, n)).astype(np.int16)
    x[1] = np.where((np.arange(n) // 40) % 2, 32767, -32768)
    taps = golden["fir/taps_am102"]
    lp = orc.biquad_design(orclib.BQ_LOWPASS, np.float32(5400 * CORR), 0.54)
    nt = orc.biquad_design(orclib.BQ_NOTCH, np.float32(3000 * CORR), 15.0)
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, taps, taps, mode=orclib.AM, biquad_nodes=[[lp], [nt]])
    got = run_chain(ctx, chain, x, np.int16, block, node_kernel="chain_q15mb_kernel" if block == B else "biquad_teensy_pipe4_kernel<2,%d>" % per_group)
    for c in (0, 1, 63, 64, 127):
        want = orc.chain_q15(x[c], orclib.AM, taps, taps, biquads=[orc.biquad_teensy_new([lp]), orc.biquad_teensy_new([nt])])
        assert np.array_equal(got[c], want), (block, c)


@pytest.mark.parametrize("ch", [16, 48, 80])
def test_chain_q15_node_slab_pipeline_on_multiples_of_16_channels(ctx, orc, golden, ch):
    """Small batches take 16 channels per workgroup on the node pipeline: channel counts that are no multiple of 64, every channel checked."""
    rng = np.random.default_rng(ch)
    n = 6 * B
    x = rng.integers(-32768, 32768, (ch, n)).astype(np.int16)
    taps = golden["fir/taps_am102"]
    lp = orc.biquad_design(orclib.BQ_LOWPASS, np.float32(5400 * CORR), 0.54)
    nt = orc.biquad_design(orclib.BQ_NOTCH, np.float32(3000 * CORR), 15.0)
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, taps, taps, mode=orclib.AM, biquad_nodes=[[lp], [nt]])
    got = run_chain(ctx, chain, x, np.int16, 2 * B, node_kernel="biquad_teensy_pipe4_kernel<2,16>")
    for c in range(ch):
        want = orc.chain_q15(x[c], orclib.AM, taps, taps, biquads=[orc.biquad_teensy_new([lp]), orc.biquad_teensy_new([nt])])
        assert np.array_equal(got[c], want), c


@pytest.mark.parametrize("variant", ["fs4", "swapped", "minus32768", "gaps", "period8"])
def test_chain_q15_nco_tables_on_matrix_cores(ctx, orc, golden, variant):
    """AudioEffectFreqConv tables of period 4 with alternating zeros (the node driven at fs/4) run on the matrix-core kernel:
    arm_mult_q15 (saturating) is applied when the samples are staged.  Other tables keep the VALU kernel.  Ragged blocks
    advance the oscillator phase between calls."""
    L = 128
    k = np.arange(L)
    c4 = {"fs4": ([32767, 0, -32767, 0], [0, 32767, 0, -32767]),
          "swapped": ([0, 30000, 0, -30000], [-20000, 0, 20000, 0]),          # osc_q at the odd phases, osc_i at the even ones
          "minus32768": ([-32768, 0, 32767, 0], [0, -32768, 0, -32768]),      # x = -32768 saturates in arm_mult_q15
          "gaps": ([32767, 0, 0, 0], [0, 0, 0, -12345])}                        # phases that feed nothing
    if variant == "period8":
        oq = np.round(32767 * np.cos(2 * np.pi * k / 8)).astype(np.int16)
        oi = np.round(32767 * np.sin(2 * np.pi * k / 8)).astype(np.int16)
    else:
        oq = np.array(c4[variant][0], np.int16)[k % 4]
        oi = np.array(c4[variant][1], np.int16)[k % 4]
    rng = np.random.default_rng(len(variant))
    ch, n = 3, 24 * B
    x = rng.integers(-32768, 32768, (ch, n)).astype(np.int16)
    x[1, ::5] = -32768
    hi, hq = golden["taps/FIR_SSB_I_coeffs"], golden["taps/FIR_SSB_Q_coeffs"]
    modes = np.array([orclib.LSB, orclib.AM, orclib.USB], np.int32)
    for flags in (0, msdr.CHAIN_NO_MFMA):
        chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, hi, hq, mixer=msdr.MIXER_NCO, modes=modes, osc_i=oi, osc_q=oq, flags=flags)
        got = np.empty_like(x)
        o = 0
        for m in [130, 7, 1025, 1, 2, 129, 3, n]:
            m = min(m, n - o)
            dx, dy = ctx.to_device(x[:, o:o + m]), ctx.array((ch, m), np.int16)
            chain.process(dx, dy, m)
            got[:, o:o + m] = dy.download()
            o += m
            if o >= n:
                break
        # (period 8 is not the fs/4 special case: it takes the full-rate layout of the same kernel)
        assert chain.info()["kernel"] == (VALU if flags else QM + " full-rate NCO streams" if variant == "period8" else QM)
        for c in range(ch):
            assert np.array_equal(got[c], orc.chain_q15(x[c], modes[c], hi, hq, mixer=1, osc_i=oi, osc_q=oq)), (variant, flags, c)


def test_chain_c1_shape_one_am_channel_block_cadence(ctx, orc, golden):
    """BASELINE configs[0]: 1 AM channel, 128-sample AudioStream blocks, 61-tap low-pass (62 taps with the designer's zero pad),
    envelope demodulator, 4-stage biquad (the Linkwitz-Riley set of Minimal-SDR.ino:393-399) -- block by block, both flavours."""
    rng = np.random.default_rng(1)
    nblk = 100
    n = np.arange(nblk * B)
    x = np.round(12000 * (0.5 + 0.4 * np.sin(2 * np.pi * 300 * n / 24000)) * np.cos(2 * np.pi * 6000 * n / 24000)) + rng.integers(-200, 201, n.size)
    x = x.astype(np.int16)[None, :]
    taps = golden["fir/taps_lp62"]
    lr = [orc.biquad_design(orclib.BQ_LOWPASS, np.float32(5400 * CORR), q) for q in (0.54, 1.3, 0.54, 1.3)]
    # Q15, as the reference runs it
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, 1, taps, taps, mode=orclib.AM, biquad_nodes=[lr])
    got = run_chain(ctx, chain, x, np.int16, B)
    want = orc.chain_q15(x[0], orclib.AM, taps, taps, biquads=[orc.biquad_teensy_new(lr)])
    assert np.array_equal(got[0], want)
    assert np.abs(want[20 * B:].astype(int)).max() > 1000                       # the envelope is there
    # fp32 (arm_fir_f32 / arm_biquad_cascade_df1_f32 semantics), same taps and sections as floats
    tf = (taps.astype(np.float64) / 32768.0).astype(np.float32)
    bq = np.array([[c[0], c[1], c[2], -c[3], -c[4]] for c in (np.asarray(s, np.float64) / 2 ** 30 for s in lr)], np.float32)   # CMSIS adds the feedback terms
    cos4, sin4 = np.array([1, 0, -1, 0], np.float32), np.array([0, 1, 0, -1], np.float32)
    chain2 = msdr.Chain(ctx, msdr.ARITH_F32, 1, tf, tf, mode=orclib.AM, biquad_coeffs=bq)
    got2 = run_chain(ctx, chain2, x, np.float32, B)
    st = {}
    want2 = np.concatenate([orc.chain_f32(x[0, b * B:(b + 1) * B], orclib.AM, tf, tf, sin4, cos4, bq, state=st) for b in range(nblk)])
    assert rel_rms(got2[0], want2) < 1e-5


@pytest.mark.parametrize("mode", [orclib.AM, orclib.LSB])
@pytest.mark.parametrize("spec", [[(1, 300, 0.7), (1, 300, 0.7)], [(1, 300, 0.7)], [(3, 1000, 8), (3, 2000, 8), (3, 3000, 8), (3, 4000, 8)]])
def test_chain_f32_ill_conditioned_cascade_runs_in_cmsis_order(ctx, orc, mode, spec):
    """Stacked high-pass / narrow-notch sections behind an envelope: the chain measures the cascade's conditioning and applies
    arm_biquad_cascade_df1_f32 as written behind the main kernel (the parallel evaluation measured 8e-3 on the first case)."""
    rng = np.random.default_rng(17)
    k = np.arange(100)
    proto = np.sinc(1920 / 24000 * (k - 49.5)) * np.kaiser(100, 6.0)
    proto /= proto.sum()
    hi = (2 * proto * np.cos(2 * np.pi * 1330 / 24000 * (k - 49.5) + np.pi / 4)).astype(np.float32)
    hq = (2 * proto * np.cos(2 * np.pi * 1330 / 24000 * (k - 49.5) - np.pi / 4)).astype(np.float32)
    cos4, sin4 = np.array([1, 0, -1, 0], np.float32), np.array([0, 1, 0, -1], np.float32)
    rows = []
    for kind, f, q in spec:
        c_ = orc.biquad_design(kind, np.float32(f * CORR), q).astype(np.float64) / 2 ** 30
        rows.append([c_[0], c_[1], c_[2], -c_[3], -c_[4]])
    bq = np.array(rows, np.float32)
    ch, n = 5, 40 * B
    x = rng.integers(-12000, 12001, (ch, n)).astype(np.int16)
    chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, hi, hq, mode=mode, biquad_coeffs=bq)
    got = run_chain(ctx, chain, x, np.float32, 13 * B + 2)
    assert chain.info()["kernel"].endswith("biquad_df1_seq_kernel")
    for c in range(ch):
        want = orc.chain_f32(x[c], mode, hi, hq, sin4, cos4, bq)
        assert rel_rms(got[c], want) < TOL, (spec, c, rel_rms(got[c], want))
    chain.reset()
    got2 = run_chain(ctx, chain, x, np.float32, None)
    assert rel_rms(got2[0], orc.chain_f32(x[0], mode, hi, hq, sin4, cos4, bq)) < TOL


@pytest.mark.parametrize("P,cycles", [(8, 1), (8, 3), (16, 5), (32, 7), (32, 13), (64, 9)])
def test_chain_f32_longer_oscillator_periods_on_matrix_cores(ctx, orc, P, cycles):
    """AudioEffectFreqConv tables of period 8, 16, 32 (any frequency cycles * fs / P): the matrix-core kernel takes one folded table
    per starting phase (the period must divide the 32-sample output row); period 64 runs the full-rate layout.  SSB and envelope
    channels, ragged calls."""
    rng = np.random.default_rng(P + cycles)
    k = np.arange(128)
    oi = (np.round(32767 * np.sin(2 * np.pi * cycles * k / P)).astype(np.int16) / 32768.0).astype(np.float32)
    oq = (np.round(32767 * np.cos(2 * np.pi * cycles * k / P)).astype(np.int16) / 32768.0).astype(np.float32)
    hi, hq = _hilbert_pair(100)
    bq = _f32_biquads(orc, 2)
    modes = np.array([orclib.LSB, orclib.USB, orclib.AM, orclib.LSB], np.int32)
    ch, n = 4, 30 * B
    x = rng.integers(-12000, 12001, (ch, n)).astype(np.int16)
    chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, hi, hq, mixer=msdr.MIXER_NCO, modes=modes, osc_i=oi, osc_q=oq, biquad_coeffs=bq,
                       flags=msdr.CHAIN_FOLD_ANY_PERIOD)
    got = np.empty((ch, n), np.float32)
    o = 0
    for m in (130, 7, 1025, 1, 2, 129, 3, n):
        m = min(m, n - o)
        dx, dy = ctx.to_device(np.ascontiguousarray(x[:, o:o + m])), ctx.array((ch, m), np.float32)
        chain.process(dx, dy, m)
        got[:, o:o + m] = dy.download()
        o += m
        if o >= n:
            break
    assert chain.info()["kernel"].startswith("chain_mfw_kernel"), chain.info()["kernel"]
    assert ("full-rate" in chain.info()["kernel"]) == (P > 32)                # period 64: the two mixer products as full-rate streams
    for c in range(ch):
        want = orc.chain_f32(x[c], modes[c], hi, hq, oi, oq, bq)
        assert rel_rms(got[c], want) < TOL, (P, c, rel_rms(got[c], want))


def test_chain_f32_cmsis_order_cascade_on_one_long_stream(ctx, orc):
    """An AM channel with a 300 Hz high-pass pair behind the envelope (DC removal: ill-conditioned for the parallel IIR), ONE
    channel, two calls of ~2^20 samples: the CMSIS-order cascade behind the main kernel runs in time segments, in place on the
    audio buffer, state carried between the calls."""
    rng = np.random.default_rng(23)
    k = np.arange(100)
    proto = np.sinc(1920 / 24000 * (k - 49.5)) * np.kaiser(100, 6.0)
    lp = (proto / proto.sum()).astype(np.float32)
    cos4, sin4 = np.array([1, 0, -1, 0], np.float32), np.array([0, 1, 0, -1], np.float32)
    c_ = orc.biquad_design(orclib.BQ_HIGHPASS, np.float32(300 * CORR), 0.7).astype(np.float64) / 2 ** 30
    bq = np.array([[c_[0], c_[1], c_[2], -c_[3], -c_[4]]] * 2, np.float32)
    lens = [(1 << 20) + 5 * B, (1 << 20) - 3 * B]
    t = np.arange(sum(lens))
    x = (np.round(9000 * (1 + 0.5 * np.cos(2 * np.pi * 700 * t / 24000)) * np.cos(2 * np.pi * 6000 * t / 24000))
         + rng.integers(-300, 301, t.size)).astype(np.int16)[None, :]
    chain = msdr.Chain(ctx, msdr.ARITH_F32, 1, lp, lp, mode=orclib.AM, biquad_coeffs=bq)
    st, o = {}, 0
    for m in lens:
        seg = np.ascontiguousarray(x[:, o:o + m])
        got = run_chain(ctx, chain, seg, np.float32)
        assert chain.info()["kernel"].endswith("biquad_df1_seq_kernel")
        want = orc.chain_f32(seg[0], orclib.AM, lp, lp, sin4, cos4, bq, state=st)
        assert rel_rms(got[0], want) < TOL, (o, rel_rms(got[0], want))
        o += m


@pytest.mark.parametrize("stages", [0, 1, 2, 4])
@pytest.mark.parametrize("kind", ["p3", "p5", "p64", "p128", "drift"])
def test_chain_f32_any_freq_conv_table_on_matrix_cores(ctx, orc, kind, stages):
    """AudioEffectFreqConv's tables are one block long (128 entries, freq_conv.h:33-34) and re-used every block (freq_conv.cpp:67-103),
    so WHATEVER is in them the oscillator sequence repeats with the block: nominal periods 3 and 5 (which do not divide 128: the
    table restarts mid-cycle at every block, as the reference would), 64, 128, and a table with no structure at all.  The
    matrix-core kernel stages the two mixer products as full-rate streams and runs both FIRs over every sample.  Mixed modes,
    ragged calls, a retune in the middle."""
    rng = np.random.default_rng({"p3": 3, "p5": 5, "p64": 64, "p128": 128, "drift": 7}[kind] + stages)
    k = np.arange(128)
    if kind == "drift":
        ph = np.cumsum(rng.uniform(0.2, 0.9, 128))
        oi, oq = np.sin(ph), np.cos(ph) * 0.9
    else:
        P = int(kind[1:])
        cyc = {3: 1, 5: 2, 64: 9, 128: 37}[P]
        oi, oq = np.sin(2 * np.pi * cyc * k / P), np.cos(2 * np.pi * cyc * k / P)
    oi = (np.round(32767 * oi).astype(np.int16) / 32768.0).astype(np.float32)
    oq = (np.round(32767 * oq).astype(np.int16) / 32768.0).astype(np.float32)
    hi, hq = _hilbert_pair(100)
    bq = _f32_biquads(orc, stages) if stages else None
    modes = np.array([orclib.LSB, orclib.USB, orclib.AM, orclib.LSB, orclib.CW], np.int32)
    ch, n = 5, 40 * B
    x = rng.integers(-12000, 12001, (ch, n)).astype(np.int16)
    chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, hi, hq, mixer=msdr.MIXER_NCO, modes=modes, osc_i=oi, osc_q=oq, biquad_coeffs=bq)
    got = np.empty((ch, n), np.float32)
    st = [dict() for _ in range(ch)]
    want = np.empty((ch, n), np.float32)
    o = 0
    for j, m in enumerate((130, 7, 1025, 1, 2, 2049, 3, n)):
        m = min(m, n - o)
        if j == 5:
            chain.set_mode(3, orclib.USB, 0)                    # a retune between calls: FIR history and cascade state carry on
            modes[3] = orclib.USB
        dx, dy = ctx.to_device(np.ascontiguousarray(x[:, o:o + m])), ctx.array((ch, m), np.float32)
        chain.process(dx, dy, m)
        got[:, o:o + m] = dy.download()
        for c in range(ch):
            want[c, o:o + m] = orc.chain_f32(x[c, o:o + m], modes[c], hi, hq, oi, oq, bq, state=st[c])
        o += m
        if o >= n:
            break
    assert "full-rate" in chain.info()["kernel"], chain.info()["kernel"]
    for c in range(ch):
        assert rel_rms(got[c], want[c]) < TOL, (kind, stages, c, rel_rms(got[c], want[c]))


@pytest.mark.parametrize("kind", ["p3", "p5", "p64", "p128", "drift", "fullscale"])
def test_chain_q15_any_freq_conv_table_on_matrix_cores(ctx, orc, golden, kind):
    """The Q15 chain with AudioEffectFreqConv tables that are NOT the fs/4 special case: the tables repeat with the 128-sample block
    whatever is in them (freq_conv.cpp:67-103), arm_mult_q15 (saturating) is applied when the samples are staged, and both filters
    run over every sample on the integer matrix cores -- bit-exact, -32768 samples and table entries included, ragged calls,
    biquad nodes behind, both envelope flavours, and against the vector-ALU kernel."""
    rng = np.random.default_rng({"p3": 3, "p5": 5, "p64": 64, "p128": 128, "drift": 7, "fullscale": 9}[kind])
    k = np.arange(128)
    if kind == "drift":
        ph = np.cumsum(rng.uniform(0.2, 0.9, 128))
        oi, oq = np.round(32767 * np.sin(ph)), np.round(29000 * np.cos(ph))
    elif kind == "fullscale":
        oi, oq = rng.choice([-32768, 32767, -1, 0, 1, 12345], 128), rng.choice([-32768, 32767, 0, 77], 128)
    else:
        P = int(kind[1:])
        cyc = {3: 1, 5: 2, 64: 9, 128: 37}[P]
        oi, oq = np.round(32767 * np.sin(2 * np.pi * cyc * k / P)), np.round(32767 * np.cos(2 * np.pi * cyc * k / P))
    oi, oq = oi.astype(np.int16), oq.astype(np.int16)
    ch, n = 4, 24 * B
    x = rng.integers(-32768, 32768, (ch, n)).astype(np.int16)
    x[1, ::5] = -32768
    hi, hq = golden["taps/FIR_SSB_I_coeffs"], golden["taps/FIR_SSB_Q_coeffs"]
    modes = np.array([orclib.LSB, orclib.AM, orclib.USB, orclib.CW], np.int32)
    lp, nt = _ref_nodes(orc)
    for flags, sqrt_kind in ((0, msdr.SQRT_F32), (0, msdr.SQRT_Q31), (msdr.CHAIN_NO_MFMA, msdr.SQRT_F32)):
        chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, hi, hq, mixer=msdr.MIXER_NCO, modes=modes, osc_i=oi, osc_q=oq, flags=flags,
                           sqrt_kind=sqrt_kind, biquad_nodes=[[lp], [nt]])
        got = np.empty_like(x)
        o = 0
        for m in [130, 6, 1026, 2, 2, 128, 4, n]:
            m = min(m, n - o)
            dx, dy = ctx.to_device(x[:, o:o + m]), ctx.array((ch, m), np.int16)
            chain.process(dx, dy, m)
            got[:, o:o + m] = dy.download()
            o += m
            if o >= n:
                break
        assert ("full-rate" in chain.info()["kernel"]) == (flags == 0), chain.info()["kernel"]
        for c in range(ch):
            want = orc.chain_q15(x[c], modes[c], hi, hq, mixer=1, osc_i=oi, osc_q=oq, sqrt_kind=sqrt_kind,
                                 biquads=[orc.biquad_teensy_new([lp]), orc.biquad_teensy_new([nt])])
            assert np.array_equal(got[c], want), (kind, flags, sqrt_kind, c)
