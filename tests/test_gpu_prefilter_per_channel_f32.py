"""Two-stage decimation for the fp32 down-converter bank: msdr_chain_set_prefilter_f32(D1, taps) in front of every receiver's channel pair;
chain_f32pcn2_kernel (the cases of tests/test_gpu_prefilter_per_channel.py).

Every channel is judged on its own by cx_cases.judge_f32 -- e_go < 1e-5 against the fp32 composition of the oracle's stages
(tests/prefilter_model.py), e_gpu <= 2 e_orc + 1e-6 against the same composition in float64, e_orc < 2e-6 (which
tests/test_prefilter_model.py shows for these inputs without a GPU); the pairs behind the channel filter are held to the 1e-5 of the I/Q tests."""
import ctypes as C

import numpy as np
import pytest

import cx_cases
import orclib
import prefilter_model as pm
from gpuhelp import ctx, msdr  # noqa: F401
from test_gpu_decim_per_channel import decim_run, guarded_call
from test_gpu_nco_per_channel import Bank, off_grid_steps, u32
from test_gpu_nco_per_channel_f32 import any_table
from test_gpu_osc_per_channel_f32 import bw_taps, mixed_bank, signal

pytestmark = pytest.mark.gpu
PCN2 = "chain_f32pcn2_kernel"
AM, LSB, USB = orclib.AM, orclib.LSB, orclib.USB
F = np.float32
BASE = msdr.FLAVOUR_PREFILTER | msdr.FLAVOUR_DECIMATED | msdr.FLAVOUR_NCO_PC | msdr.FLAVOUR_TAPS_PC


def nco_chain(ctx, ch, ti, tq, steps, phases, **kw):
    chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, ti[0], tq[0], mixer=msdr.MIXER_NCO, **any_table(), **kw)
    chain.set_taps_channels_f32(0, ti, tq)
    chain.set_nco_channels(0, u32(steps), u32(phases))
    return chain


def pre_chain(ctx, ch, ti, tq, steps, phases, modes, p, D1, D2, **kw):
    chain = nco_chain(ctx, ch, ti, tq, steps, phases, modes=modes, **kw)
    chain.set_prefilter(D1, p)
    if D2 > 1:
        chain.set_decimation(D2)
    assert chain.prefilter() == (D1, p.size) and chain.decimation() == D2
    return chain


def refs(orc, x, si, sq, p, D1, modes, ti, tq, D2):
    """per channel: ((audio, fi, fq) fp32, (audio, fi, fq) float64)"""
    return [(pm.model_f32(orc, x[c], si[c], sq[c], p, D1, modes[c], ti[c], tq[c], D2), pm.model_f64(x[c], si[c], sq[c], p, D1, modes[c], ti[c], tq[c], D2))
            for c in range(len(modes))]


def judge(tag, got, r, lo=0, hi=None):
    for c, (w32, t64) in enumerate(r):
        cx_cases.judge_f32("%s ch %d" % (tag, c), got[c], w32[0][lo:hi], t64[0][lo:hi])


# ------------------------------------------------------------------------------------------------ 1. the oracle, every geometry and call split
@pytest.mark.parametrize("shape", pm.SHAPES)
def test_oracle_every_geometry(ctx, orc, shape):
    D1, N1, D2 = shape
    k = pm.case_f32(shape)
    ch = k["x"].shape[0]
    r = refs(orc, k["x"], k["si"], k["sq"], k["p"], D1, k["modes"], k["ti"], k["tq"], D2)
    outs = []
    for nout, tile in zip(pm.NOUTS, pm.TILES["f32"][shape]):
        chain = pre_chain(ctx, ch, k["ti"], k["tq"], k["steps"], k["phases"], k["modes"], k["p"], D1, D2)
        got = decim_run(ctx, chain, k["x"], nout * D1 * D2, D1 * D2, F)
        info = chain.info()
        assert info["kernel"].startswith(PCN2) and info["tile"] == tile, (nout, info)
        assert info["flavour"] & BASE == BASE and info["flavour"] & 0x8000000, info
        assert not info["flavour"] & (msdr.FLAVOUR_BLOCK | msdr.FLAVOUR_OSC_PC | msdr.FLAVOUR_COMPLEX_IN | msdr.FLAVOUR_GAIN), info
        g = pm.geometry(True, pm.pad(N1, True), D1, 104, D2, nout, ch, 256)
        assert info["lds_bytes"] == g["lds_bytes"] and info["block"] == g["block"], (nout, info, g)
        judge("%s nout %d" % (shape, nout), got, r)
        outs.append(got)
        chain.close()
    # a tile recomputes what it shares with its neighbour from raw samples, in one order: the split into calls changes no bit
    print("prefilter f32 %s: call splits bit-identical: %s" % (shape, [bool(np.array_equal(o.view(np.uint32), outs[0].view(np.uint32))) for o in outs[1:]]))


def test_one_call_in_time_segments(ctx, orc):
    shape = pm.SEGMENTED["shape"]
    D1, N1, D2 = shape
    k = pm.case_f32(shape, pm.SEGMENTED["nout"])
    ch = k["x"].shape[0]
    chain = pre_chain(ctx, ch, k["ti"], k["tq"], k["steps"], k["phases"], k["modes"], k["p"], D1, D2)
    got = decim_run(ctx, chain, k["x"], k["x"].shape[1], D1 * D2, F)
    info = chain.info()
    assert info["kernel"].startswith(PCN2) and info["tile"] == pm.SEGMENTED["tile"]["f32"] and info["time_segments"] == pm.SEGMENTED["nseg"]["f32"] >= 2, info
    assert info["flavour"] & msdr.FLAVOUR_SEGMENTED, info
    judge("segments", got, refs(orc, k["x"], k["si"], k["sq"], k["p"], D1, k["modes"], k["ti"], k["tq"], D2))
    chain.close()


# ------------------------------------------------------------------------------------------------ 2. guards and pairs
def test_nothing_is_written_past_the_rows_of_audio_and_pairs(ctx, orc):
    D1, N1, D2 = 4, 16, 4
    rng = np.random.default_rng(3402)
    ch = 11
    modes, ti, tq = mixed_bank(ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    p = pm.lowpass(D1, N1, F)
    for nout in (32, 200):
        x = signal(rng, ch, nout * D1 * D2)
        a = pre_chain(ctx, ch, ti, tq, steps, phases, modes, p, D1, D2)
        pitch = (nout + 7) // 8 * 8 + 8
        buf = ctx.to_device(np.full((ch + 2) * pitch * 2, -7.0, F))
        a.set_iq_out(buf.offset(pitch * 8), pitch)
        got, intact = guarded_call(ctx, a, x, D1 * D2, ch, F, F(-7.0))
        assert intact, nout
        assert a.info()["flavour"] & (BASE | msdr.FLAVOUR_IQ_OUT) == BASE | msdr.FLAVOUR_IQ_OUT
        pairs = buf.download().reshape(ch + 2, pitch, 2)
        assert (pairs[0] == -7.0).all() and (pairs[-1] == -7.0).all() and (pairs[1:-1, nout:] == -7.0).all(), nout
        si, sq = Bank(steps, phases).advance(x.shape[1])
        r = refs(orc, x, si, sq, p, D1, modes, ti, tq, D2)
        judge("guards nout %d" % nout, got, r)
        for c in range(ch):
            for j, name in ((0, "fi"), (1, "fq")):
                e = cx_cases.rel(pairs[1 + c, :nout, j], r[c][0][1 + j])
                print("prefilter f32 pairs nout %d ch %d %s %.3e" % (nout, c, name, e))
                assert e < 1e-5, (nout, c, name, e)
        a.close()


# ------------------------------------------------------------------------------------------------ 3. live changes between calls
def test_a_retune_and_a_tap_change_between_calls(ctx, orc):
    D1, N1, D2 = 8, 32, 4
    rng = np.random.default_rng(3403)
    ch, calls, nout = 6, 6, 64
    step = nout * D1 * D2
    n = calls * step
    modes = np.array([AM, LSB, AM, USB, AM, LSB], np.int32)
    t0 = np.stack([bw_taps(600.0 + 500.0 * c) for c in range(ch)])
    t1 = np.stack([bw_taps(2900.0 - 300.0 * c) for c in range(ch)])
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    new_steps = off_grid_steps(rng, 3)
    p = pm.lowpass(D1, N1, F)
    x = signal(rng, ch, n)
    chain = pre_chain(ctx, ch, t0, t0, steps, phases, modes, p, D1, D2)
    bank = Bank(steps, phases)
    got, si, sq = [], [], []
    for k in range(calls):
        if k == 2:
            chain.set_nco_channels(1, u32(new_steps))
            bank.retune(1, new_steps)
        if k == 4:
            chain.set_taps_channels_f32(2, t1[2:5], t1[2:5])
        got.append(decim_run(ctx, chain, x[:, k * step:(k + 1) * step], step, D1 * D2, F))
        a, b = bank.advance(step)
        si.append(a)
        sq.append(b)
        bank.check(chain, k)
    got, si, sq = np.concatenate(got, 1), np.concatenate(si, 1), np.concatenate(sq, 1)
    assert chain.info()["kernel"].startswith(PCN2)
    for c in range(ch):
        w32 = pm.model_f32(orc, x[c], si[c], sq[c], p, D1, modes[c], t0[c], t0[c], D2)[0]
        t64 = pm.model_f64(x[c], si[c], sq[c], p, D1, modes[c], t0[c], t0[c], D2)[0]
        if 2 <= c < 5:
            w32 = np.concatenate([w32[:4 * nout], pm.model_f32(orc, x[c], si[c], sq[c], p, D1, modes[c], t1[c], t1[c], D2)[0][4 * nout:]])
            t64 = np.concatenate([t64[:4 * nout], pm.model_f64(x[c], si[c], sq[c], p, D1, modes[c], t1[c], t1[c], D2)[0][4 * nout:]])
        cx_cases.judge_f32("live ch %d" % c, got[c], w32, t64)
    chain.close()


def test_reset_and_init_fir(ctx, orc):
    D1, N1, D2 = 4, 16, 4
    rng = np.random.default_rng(3404)
    ch, nout = 5, 96
    n = nout * D1 * D2
    modes, ti, tq = mixed_bank(ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    p = pm.lowpass(D1, N1, F)
    x = signal(rng, ch, 3 * n)
    chain = pre_chain(ctx, ch, ti, tq, steps, phases, modes, p, D1, D2)
    bank = Bank(steps, phases)
    for k in range(3):
        if k == 1:
            chain.init_fir()
        if k == 2:
            chain.reset()
            bank.reset()
        got = decim_run(ctx, chain, x[:, k * n:(k + 1) * n], n // 2, D1 * D2, F)
        si, sq = bank.advance(n)
        judge("part %d" % k, got, refs(orc, x[:, k * n:(k + 1) * n], si, sq, p, D1, modes, ti, tq, D2))
        assert chain.prefilter() == (D1, N1) and chain.decimation() == D2
    chain.close()


def test_set_decimation_switched_between_calls(ctx, orc):
    D1, N1 = 4, 16
    rng = np.random.default_rng(3405)
    ch, inter = 5, 96 * 12
    step = inter * D1
    seq = (4, 3, 1, 4)
    n = len(seq) * step
    modes, ti, tq = mixed_bank(ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    p = pm.lowpass(D1, N1, F)
    x = signal(rng, ch, n)
    si, sq = Bank(steps, phases).advance(n)
    full = refs(orc, x, si, sq, p, D1, modes, ti, tq, 1)          # the channel pair's output at fs / D1: one stream, picked every D2-th
    chain = pre_chain(ctx, ch, ti, tq, steps, phases, modes, p, D1, 1)
    for k, D2 in enumerate(seq):
        chain.set_decimation(D2)
        got = decim_run(ctx, chain, x[:, k * step:(k + 1) * step], step, D1 * D2, F)
        assert chain.info()["kernel"].startswith(PCN2)
        pick = np.arange(k * inter + D2 - 1, (k + 1) * inter, D2)
        for c in range(ch):
            cx_cases.judge_f32("D2 %d call %d ch %d" % (D2, k, c), got[c], full[c][0][0][pick], full[c][1][0][pick])
    chain.close()


# ------------------------------------------------------------------------------------------------ 4. one antenna row
@pytest.mark.parametrize("ch", [1, 5, 17])
def test_a_shared_antenna_row(ctx, orc, ch):
    D1, N1, D2 = 8, 32, 4
    rng = np.random.default_rng(3406 + ch)
    nout = 160
    n = nout * D1 * D2
    modes, ti, tq = mixed_bank(ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    p = pm.lowpass(D1, N1, F)
    x = signal(rng, 1, n)
    si, sq = Bank(steps, phases).advance(n)
    chain = pre_chain(ctx, ch, ti, tq, steps, phases, modes, p, D1, D2)
    chain.set_input_rows(np.zeros(ch, np.int64), 1)
    got = decim_run(ctx, chain, x, n // 2, D1 * D2, F, channels=ch)
    info = chain.info()
    assert info["kernel"].startswith(PCN2) and info["flavour"] & msdr.FLAVOUR_SHARED_IF, info
    judge("shared %d" % ch, got, refs(orc, np.repeat(x, ch, 0), si, sq, p, D1, modes, ti, tq, D2))
    chain.close()


# ------------------------------------------------------------------------------------------------ 5. the delta prefilter and the one-stage kernel
@pytest.mark.parametrize("D1,D2", [(4, 4), (2, 3)])
def test_the_delta_prefilter_against_the_one_stage_kernel_with_zero_stuffed_taps(ctx, orc, D1, D2):
    rng = np.random.default_rng([3407, D1, D2])
    ch, nout = 7, 200
    n = nout * D1 * D2
    modes, ti, tq = mixed_bank(ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    x = signal(rng, ch, n)
    si, sq = Bank(steps, phases).advance(n)
    p = pm.delta(D1, F)
    two = pre_chain(ctx, ch, ti, tq, steps, phases, modes, p, D1, D2)
    zi, zq = np.stack([pm.zero_stuff(t, D1) for t in ti]), np.stack([pm.zero_stuff(t, D1) for t in tq])
    one = nco_chain(ctx, ch, zi, zq, steps, phases, modes=modes)
    one.set_decimation(D1 * D2)
    a, b = decim_run(ctx, two, x, n, D1 * D2, F), decim_run(ctx, one, x, n, D1 * D2, F)
    assert two.info()["kernel"].startswith(PCN2) and one.info()["kernel"].startswith("chain_f32pcnd_kernel")
    judge("delta", a, refs(orc, x, si, sq, p, D1, modes, ti, tq, D2))
    for c in range(ch):
        cx_cases.judge_f32("delta against one stage ch %d" % c, a[c], b[c], pm.model_f64(x[c], si[c], sq[c], p, D1, modes[c], ti[c], tq[c], D2)[0])
    print("prefilter f32 delta (%d, %d): two-stage and one-stage outputs bit-identical: %s" % (D1, D2, bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))))
    two.close()
    one.close()


# ------------------------------------------------------------------------------------------------ 6. int16 out
def test_int16_output_is_within_one_lsb(ctx, orc):
    D1, N1, D2 = 4, 16, 4
    rng = np.random.default_rng(3408)
    ch, nout = 6, 200
    n = nout * D1 * D2
    modes, ti, tq = mixed_bank(ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    p = pm.lowpass(D1, N1, F)
    x = signal(rng, ch, n)
    si, sq = Bank(steps, phases).advance(n)
    chain = pre_chain(ctx, ch, ti, tq, steps, phases, modes, p, D1, D2, flags=msdr.CHAIN_OUT_I16)
    got = decim_run(ctx, chain, x, n // 2, D1 * D2, np.int16)
    assert chain.info()["kernel"].startswith(PCN2)
    for c, (w32, _) in enumerate(refs(orc, x, si, sq, p, D1, modes, ti, tq, D2)):
        want = np.clip(np.round(w32[0].astype(np.float64) * 32768.0), -32768, 32767)
        assert np.abs(got[c].astype(np.float64) - want).max() <= 1, c
        assert np.abs(got[c].astype(np.int32)).max() > 100, c
    chain.close()


# ------------------------------------------------------------------------------------------------ 7. refusals: nothing changed
def test_every_refusal_leaves_the_chain_as_it_was(ctx, orc):
    D1, N1, D2 = 4, 16, 4
    rng = np.random.default_rng(3409)
    ch, nout = 5, 64
    n = nout * D1 * D2
    modes, ti, tq = mixed_bank(ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    p = pm.lowpass(D1, N1, F)
    x = signal(rng, ch, 2 * n)
    si, sq = Bank(steps, phases).advance(2 * n)
    lib = ctx.lib

    def refused(f, *a):
        with pytest.raises(msdr.MsdrError) as e:
            f(*a)
        assert e.value.status == msdr.STATUS_ARGUMENT_ERROR, e.value
        assert "nothing changed" in str(e.value), e.value

    plain = msdr.Chain(ctx, msdr.ARITH_F32, ch, ti[0], tq[0], mixer=msdr.MIXER_NCO, modes=modes, **any_table())
    refused(plain.set_prefilter, D1, p)          # not in phase-accumulator mode
    plain.close()
    chain = nco_chain(ctx, ch, ti, tq, steps, phases, modes=modes)
    p16 = np.zeros(16, np.int16)
    assert lib.msdr_chain_set_prefilter(chain.h, C.c_uint32(D1), C.c_uint32(16), p16.ctypes.data_as(C.c_void_p)) == msdr.STATUS_ARGUMENT_ERROR          # the other arithmetic's
    assert lib.msdr_chain_set_prefilter_f32(chain.h, C.c_uint32(D1), C.c_uint32(N1), None) == msdr.STATUS_ARGUMENT_ERROR                               # a NULL row
    for bad in (np.nan, np.inf, -np.inf):
        q = p.copy()
        q[5] = bad
        refused(chain.set_prefilter, D1, q)
    for bad in (3, 6, 64):
        refused(chain.set_prefilter, bad, p)
    refused(chain.set_prefilter, 32, np.ones(20000, F))          # no geometry fits
    chain.set_complex_input(1, 0)
    refused(chain.set_prefilter, D1, p)
    chain.set_complex_input(0)
    assert chain.prefilter() == (1, 0)
    chain.set_prefilter(D1, p[:15])          # fp32 takes odd counts (padded to 16 in front)
    chain.set_prefilter(D1, p)
    refused(chain.set_complex_input, 1, 0)
    chain.set_decimation(D2)
    refused(chain.set_decimation, 52)          # fits the one-stage kernel (1024 D + 16 np <= 61 440), not beside the stage-1 chunk
    assert chain.decimation() == D2
    chain.set_block_kernel(1)                  # accepted: such calls run the unfused launches
    dx, dy = ctx.to_device(x[:, :n + 8]), ctx.array((ch, nout + 1), F)
    with pytest.raises(msdr.MsdrError) as e:
        chain.process(dx, dy, n + 8)
    assert e.value.status == msdr.STATUS_LENGTH_ERROR
    got = [decim_run(ctx, chain, x[:, :n], n, D1 * D2, F)]
    refused(chain.set_prefilter, D1, pm.lowpass(D1, 30, F))
    refused(chain.set_prefilter, 1, p)
    assert chain.prefilter() == (D1, N1)
    got.append(decim_run(ctx, chain, x[:, n:], n, D1 * D2, F))
    assert chain.info()["kernel"].startswith(PCN2)
    judge("after refusals", np.concatenate(got, 1), refs(orc, x, si, sq, p, D1, modes, ti, tq, D2))
    chain.reset()
    chain.set_prefilter(1, None)
    decim_run(ctx, chain, x[:, :n], n, D2, F)
    info = chain.info()
    assert info["kernel"].startswith("chain_f32pcnd_kernel") and not info["flavour"] & msdr.FLAVOUR_PREFILTER, info
    chain.close()
