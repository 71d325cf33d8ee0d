"""Per-receiver decimation for the fp32 chain: msdr_chain_set_decimation(D) on a chain in phase-accumulator mode; chain_f32pcnd_kernel mixes
every input sample and evaluates the FIR pair, the demodulator and the store once per D of them; the CMSIS-order cascade and the int16
conversion behind it run on n / D samples per channel.

Every channel is judged on its own through f32judge.judge, exactly as tests/test_gpu_nco_per_channel_f32.py judges the undecimated kernel:
e_go < 1e-5 against orclib.Oracle.chain_f32 and e_gpu <= 2 e_orc + fp32_noise + 1e-6 against float64 -- the same helper, the same level, no
new tolerance.  The references are the FULL-RATE streams (the oscillator values of each sample's own time, as in that file) subsampled at the
input index of every output, m D + D - 1 of each call; a cascade behind the kernel is evaluated in CMSIS order (fp32) and in float64 over
those decimated streams."""
import numpy as np
import pytest
from scipy.signal import lfilter

import cascade_pc_cases as cc
import orclib
from f32pc_cases import B, bw_taps, cascade
from gpuhelp import ctx, msdr  # noqa: F401
from test_gpu_decim_per_channel import LIVE_N, NOUTS, decim_run, guarded_call, live_stream, step_list
from test_gpu_nco_per_channel import Bank, off_grid_steps, u32
from test_gpu_nco_per_channel_f32 import any_table, f32
from test_gpu_osc_per_channel_f32 import check, mixed_bank, refs_of, signal

pytestmark = pytest.mark.gpu
PCND = "chain_f32pcnd_kernel"
AM, LSB, USB = orclib.AM, orclib.LSB, orclib.USB
BASE = msdr.FLAVOUR_DECIMATED | msdr.FLAVOUR_NCO_PC | msdr.FLAVOUR_TAPS_PC
# msdr_decpc_geometry.h at 102 taps (np = 104), 11 channels: the tile in outputs for calls of 32 / 128 / 256 / 768 outputs (an fp32 window
# sample is 4 bytes and there is one copy per stream for every D: the Q15 figures of an odd D)
TILES = {2: (128, 128, 256, 512), 3: (64, 64, 128, 512), 8: (32, 32, 64, 128), 32: (32, 32, 64, 128)}


def nco_chain(ctx, ch, ti, tq, steps, phases, **kw):
    chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, ti[0], tq[0], mixer=msdr.MIXER_NCO, **any_table(), **kw)
    chain.set_taps_channels_f32(0, ti, tq)
    chain.set_nco_channels(0, u32(steps), u32(phases))
    return chain


def subsample(refs, index):
    return tuple(r[index] for r in refs)


# ------------------------------------------------------------------------------------------------ 1. the oracle, every geometry
@pytest.mark.parametrize("D", sorted(TILES))
def test_oracle_every_geometry(ctx, orc, D):
    rng = np.random.default_rng(2200 + D)
    n = 768 * D
    steps = step_list(rng)
    ch = steps.size
    modes, ti, tq = mixed_bank(ch)
    phases = rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    x = signal(rng, ch, n)
    si, sq = Bank(steps, phases).advance(n)
    si, sq = f32(si), f32(sq)
    index = np.arange(D - 1, n, D)
    refs = [subsample(refs_of(orc, x[c], modes[c], ti[c], tq[c], si[c], sq[c], None), index) for c in range(ch)]
    for nout, tile in zip(NOUTS, TILES[D]):
        chain = nco_chain(ctx, ch, ti, tq, steps, phases, modes=modes)
        chain.set_decimation(D)
        got = decim_run(ctx, chain, x, nout * D, D, np.float32)
        info = chain.info()
        assert info["kernel"].startswith(PCND) and info["tile"] == tile, (nout, info)
        assert info["flavour"] & BASE == BASE and info["flavour"] & 0x100000, info
        assert not info["flavour"] & (msdr.FLAVOUR_SEQ_CASCADE | msdr.FLAVOUR_CASCADE_PC | msdr.FLAVOUR_BLOCK | msdr.FLAVOUR_OSC_PC), info
        for c in range(ch):
            check("D %d nout %d ch %d" % (D, nout, c), got[c], x[c], refs[c], None)
        chain.close()


# ------------------------------------------------------------------------------------------------ 3. nothing written past the row
@pytest.mark.parametrize("D", [3, 8])
def test_nothing_is_written_past_the_row(ctx, D):
    rng = np.random.default_rng(2203 + D)
    ch = 11
    modes, ti, tq = mixed_bank(ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    a, control = (nco_chain(ctx, ch, ti, tq, steps, phases, modes=modes) for _ in range(2))
    for o in (a, control):
        o.set_decimation(D)
    for nout in (32, 768):
        x = signal(rng, ch, nout * D)
        got, intact = guarded_call(ctx, a, x, D, ch, np.float32, np.float32(-7.0))          # (-7: far outside the range of the audio)
        assert intact, nout
        want = decim_run(ctx, control, x, nout * D, D, np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), nout
        assert (got != np.float32(-7.0)).all()
    a.close()
    control.close()


# ------------------------------------------------------------------------------------------------ 4. a per-channel cascade at the decimated rate
def test_a_two_stage_per_channel_cascade_behind_it(ctx, orc):
    rng = np.random.default_rng(2204)
    ch, D, calls = 6, 4, 3
    n = calls * B * D
    rows = cc.bank_rows(ch)
    taps = np.stack([bw_taps(900.0 + 400.0 * c) for c in range(ch)])
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    x = signal(rng, ch, n)
    si, sq = Bank(steps, phases).advance(n)
    si, sq = f32(si), f32(sq)
    chain = nco_chain(ctx, ch, taps, taps, steps, phases, mode=AM, biquad_coeffs=rows[0])
    chain.set_biquad_coeffs_channels(0, rows)
    chain.set_decimation(D)
    got = decim_run(ctx, chain, x, B * D, D, np.float32)
    info = chain.info()
    want_flav = BASE | msdr.FLAVOUR_SEQ_CASCADE | msdr.FLAVOUR_CASCADE_PC
    assert info["kernel"].startswith(PCND) and info["kernel"].endswith("biquad_df1_seq_pc_kernel"), info
    assert info["flavour"] & want_flav == want_flav, info
    index = np.arange(D - 1, n, D)
    for c in range(ch):
        _, truth_pre, pre = subsample(refs_of(orc, x[c], AM, taps[c], taps[c], si[c], sq[c], None), index)
        df1 = cc.Df1(rows[c])
        want = np.concatenate([df1.run(pre[k * B:(k + 1) * B]) for k in range(calls)])          # arm_biquad_cascade_df1_f32 per call, pState kept
        truth = truth_pre
        for s in rows[c].astype(np.float64):
            truth = lfilter(s[:3], [1.0, -s[3], -s[4]], truth)
        check("cascade ch %d" % c, got[c], x[c], (want, truth, pre), rows[c])
        # get_cmsis_state continues a CMSIS-order evaluation over the DECIMATED stream: the three calls are judged as one stream (pState
        # carried from call to call), and the last stage keeps the last two OUTPUTS of the decimated call
        st = chain.cmsis_state(c)
        assert st[6] == got[c, -1] and st[7] == got[c, -2], c
    chain.close()


def test_int16_output_is_within_one_lsb(ctx, orc):
    rng = np.random.default_rng(2207)
    ch, D = 6, 4
    n = 4 * B * D
    bq = cascade("lp")
    taps = np.stack([bw_taps(1500.0 + 300.0 * c) for c in range(ch)])
    steps = np.array([msdr.nco_step(6000.0 + 3.3 * c - 7.0) for c in range(ch)], np.uint64)
    phases = rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    t = np.arange(n)
    x = np.round(12000 * (1 + 0.5 * np.sin(2 * np.pi * 400 * t / 24000.0)) * np.cos(2 * np.pi * 6000.0 * t / 24000.0) + rng.normal(0, 200, (ch, n))).astype(np.int16)
    si, sq = Bank(steps, phases).advance(n)
    chain = nco_chain(ctx, ch, taps, taps, steps, phases, mode=AM, biquad_coeffs=bq, flags=msdr.CHAIN_OUT_I16)
    chain.set_decimation(D)
    got = decim_run(ctx, chain, x, B * D, D, np.int16)
    info = chain.info()
    assert info["kernel"].startswith(PCND) and info["flavour"] & (BASE | msdr.FLAVOUR_SEQ_CASCADE) == BASE | msdr.FLAVOUR_SEQ_CASCADE, info
    assert not info["flavour"] & msdr.FLAVOUR_CASCADE_PC, info
    for c in range(ch):
        pre = orc.chain_f32(x[c], AM, taps[c], taps[c], f32(si[c]), f32(sq[c]), None)[D - 1::D]
        want = cc.Df1(bq).run(pre)
        wi = np.clip(np.round(want.astype(np.float64) * 32768.0), -32768, 32767)
        assert np.abs(got[c].astype(np.float64) - wi).max() <= 1, c
        assert np.abs(got[c]).max() > 100
    chain.close()


# ------------------------------------------------------------------------------------------------ 5. live
def test_live_switches_retunes_and_a_shared_row(ctx, orc):
    rng = np.random.default_rng(2205)
    ch, nt = 6, 500
    taps = np.stack([bw_taps(600.0 + 300.0 * c, nt) for c in range(ch)])
    modes = np.array([(AM, LSB, USB, AM)[c % 4] for c in range(ch)], np.int32)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, taps[0], taps[0], mixer=msdr.MIXER_NCO, modes=modes, **any_table())
    chain.set_input_rows(np.zeros(ch, np.int64), 1)
    chain.set_nco_channels(0, u32(steps), u32(phases))
    chain.set_taps_channels_f32(0, taps)
    x = signal(rng, 1, LIVE_N)
    got, index, si, sq = live_stream(ctx, rng, chain, Bank(steps, phases), x, np.float32)
    assert chain.info()["flavour"] & msdr.FLAVOUR_SHARED_IF
    for c in range(ch):
        refs = subsample(refs_of(orc, x[0], modes[c], taps[c], taps[c], f32(si[c]), f32(sq[c]), None), index)
        check("live ch %d" % c, got[c], x[0], refs, None)
    chain.close()
