"""Complex I/Q input of the per-receiver down-converter bank (Q15): msdr_chain_set_complex_input makes the phase-accumulator kernels read rows of
pairs {I, Q} and apply freq_conv's full mix (freq_conv.cpp:67-103), in either direction.

The expected value is always composed from the oracle's own stages (tests/cx_cases.py): freqconv_q15 -> fir_q15_blocks pair -> demod_q15, with
the oscillator rows of Bank(steps, phases); everything is compared with ==."""
import numpy as np
import pytest

import orclib
from cx_cases import B, compose_q15, cx_run, interleave, out_index
from gpuhelp import ctx, msdr  # noqa: F401
from test_gpu_decim_per_channel import nco_chain, step_list
from test_gpu_iq_per_channel import bank5
from test_gpu_nco_per_channel import Bank, any_table, off_grid_steps, u32
from test_gpu_osc_per_channel import lowpass, mixed_bank

pytestmark = pytest.mark.gpu
AM, LSB, USB, CW, SYNCAM = orclib.AM, orclib.LSB, orclib.USB, orclib.CW, orclib.SYNCAM
ARG = msdr.STATUS_ARGUMENT_ERROR
I16, U64 = np.int16, np.uint64


def cx_chain(ctx, ch, ti, tq, steps, phases, modes, direction, **kw):
    chain = nco_chain(ctx, ch, ti, tq, steps, phases, modes, **kw)
    chain.set_complex_input(True, direction)
    assert chain.complex_input() == (True, direction)
    return chain


def refs(orc, xi, xq, si, sq, direction, modes, ti, tq):
    return [compose_q15(orc, xi[c], xq[c], si[c], sq[c], direction, modes[c], ti[c], tq[c]) for c in range(len(modes))]


def same(audio, pairs, want, idx, tag):
    for c, w in enumerate(want):
        assert np.array_equal(audio[c], w[0][idx]), (tag, c)
        if pairs is not None:
            assert np.array_equal(pairs[c], np.stack([w[1][idx], w[2][idx]], axis=1)), (tag, c)


def refused(f, *a):
    with pytest.raises(msdr.MsdrError) as e:
        f(*a)
    assert e.value.status == ARG, e.value


# ------------------------------------------------------------------------------------------------ 1. every sliding-window geometry
@pytest.mark.parametrize("direction", [0, 1])
def test_every_sliding_window_geometry(ctx, orc, golden, direction):
    """10 channels (partial groups at 4 and 2 channels per wave), 102 taps, AM / LSB / USB / CW / SYNCAM, off-grid steps; 768 samples as 6 x 128,
    3 x 256 and 1 x 768 (tiles 128 / 256 / 512)"""
    rng = np.random.default_rng(7100 + direction)
    ch, n = 10, 6 * B
    modes, ti, tq = bank5(golden, ch)
    assert set(modes.tolist()) == {AM, LSB, USB, CW, SYNCAM}
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=U64)
    si, sq = Bank(steps, phases).advance(n)
    xi, xq = (rng.integers(-30000, 30001, (ch, n)).astype(I16) for _ in range(2))
    want = refs(orc, xi, xq, si, sq, direction, modes, ti, tq)
    runs = []
    for step, tile in ((B, 128), (2 * B, 256), (n, 512)):
        chain = cx_chain(ctx, ch, ti, tq, steps, phases, modes, direction)
        plain, _, _ = cx_run(ctx, chain, interleave(xi, xq), step)
        same(plain, None, want, np.arange(n), ("plain", step))
        chain.reset()
        chain.set_nco_channels(0, u32(steps), u32(phases))
        audio, pairs, _ = cx_run(ctx, chain, interleave(xi, xq), step, pdtype=I16)
        info = chain.info()
        assert info["kernel"].startswith("chain_q15pcn_kernel") and info["tile"] == tile, info          # the names stay
        same(audio, pairs, want, np.arange(n), step)
        assert np.abs(pairs.astype(np.int32)).max() > 1000
        runs.append((audio, pairs))
        chain.close()
    for a, p in runs[1:]:
        assert np.array_equal(a, runs[0][0]) and np.array_equal(p, runs[0][1])


# ------------------------------------------------------------------------------------------------ 2. the saturation corner
@pytest.mark.parametrize("direction", [0, 1])
def test_the_sums_saturate_as_freq_conv_does(ctx, orc, golden, direction):
    """every xi, xq from {-32768, 32767}; oscillators near 45 and 225 degrees (c ~ s): the second saturation, that of the sum, is met"""
    rng = np.random.default_rng(7200 + direction)
    ch, n = 3, 2 * B
    modes, ti, tq = mixed_bank(golden, ch)
    steps = np.array([1, 3 << 8, 5 << 12], U64) | U64(1)
    phases = np.array([0x20000000, 0xA0000000, 0x1FFF0000], U64)
    si, sq = Bank(steps, phases).advance(n)
    xi, xq = (rng.choice(np.array([-32768, 32767], I16), (ch, n)) for _ in range(2))
    want = refs(orc, xi, xq, si, sq, direction, modes, ti, tq)
    # from the oracle alone: some sum of two (already saturated) products leaves int16, and the mixed sample sits at the rail
    sat = lambda v: np.clip(v, -32768, 32767)          # noqa: E731
    p = lambda a, b: sat((a.astype(np.int64) * b.astype(np.int64)) >> 15)          # noqa: E731
    raw_i = p(xi, sq) + (-1 if direction else 1) * p(xq, si)
    over = (raw_i > 32767) | (raw_i < -32768)
    assert over.any()
    mixed_i = np.stack([w[3] for w in want])
    assert np.array_equal(mixed_i, sat(raw_i).astype(I16))
    assert np.isin(mixed_i[over], (32767, -32768)).all()
    chain = cx_chain(ctx, ch, ti, tq, steps, phases, modes, direction)
    audio, pairs, _ = cx_run(ctx, chain, interleave(xi, xq), B, pdtype=I16)
    same(audio, pairs, want, np.arange(n), "rails")
    chain.close()


# ------------------------------------------------------------------------------------------------ 3. the tail and the segments
@pytest.mark.parametrize("n", [1001, 4600])
def test_the_tail_and_the_segments(ctx, orc, golden, n):
    rng = np.random.default_rng(7300 + n)
    ch = 3
    modes, ti, tq = mixed_bank(golden, ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=U64)
    si, sq = Bank(steps, phases).advance(n)
    xi, xq = (rng.integers(-30000, 30001, (ch, n)).astype(I16) for _ in range(2))
    chain = cx_chain(ctx, ch, ti, tq, steps, phases, modes, 0)
    audio, pairs, _ = cx_run(ctx, chain, interleave(xi, xq), n, pdtype=I16)
    info = chain.info()
    assert info["tile"] == 512 and (info["time_segments"] >= 2) == (n == 4600), info
    same(audio, pairs, refs(orc, xi, xq, si, sq, 0, modes, ti, tq), np.arange(n), n)
    chain.close()


# ------------------------------------------------------------------------------------------------ 4. decimation
@pytest.fixture(scope="module")
def dec_ref(orc, golden):
    """one full-rate reference for every factor: 11 channels (step_list), mixed modes, 301 * 32 samples, dir 0"""
    rng = np.random.default_rng(7400)
    steps = step_list(rng)
    ch = steps.size
    modes, ti, tq = mixed_bank(golden, ch)
    phases = rng.integers(0, 1 << 32, ch, dtype=U64)
    n = 301 * 32
    xi, xq = (rng.integers(-30000, 30001, (ch, n)).astype(I16) for _ in range(2))
    si, sq = Bank(steps, phases).advance(n)
    return dict(steps=steps, phases=phases, modes=modes, ti=ti, tq=tq, x=interleave(xi, xq), want=refs(orc, xi, xq, si, sq, 0, modes, ti, tq), ch=ch)


@pytest.mark.parametrize("D", [2, 3, 4, 8, 32])
def test_decimation(ctx, dec_ref, D):
    """odd D: two window copies (AL 0); 2, 4, 8, 32: AL 1, 2, 4, 4.  256 D inputs in calls of 32 and 128 outputs (4 channels per wave) and one of
    256 (2 per wave); one call of 301 outputs -- not a multiple of any tile: a partial last tile -- at 1 channel per wave; meter and I/Q
    buffer both set.  So every launch here is the _cx_iq_meter twin: its 12 (CPW, AL) instantiations are met, at 102 taps (no CPW lowered by the LDS fit); the
    36 of the plain, metered and I/Q twins are not (test_one_channel_per_wave_decimated adds one of them).  tests/test_gpu_cx_census.py holds
    all 48, under every launch geometry"""
    r = dec_ref
    cpws = set()
    for nout in (32, 128, 256, 301):
        chain = cx_chain(ctx, r["ch"], r["ti"], r["tq"], r["steps"], r["phases"], r["modes"], 0)
        chain.set_decimation(D)
        m = (301 if nout == 301 else 256) * D
        audio, pairs, meters = cx_run(ctx, chain, r["x"][:, :m], nout * D, D, pdtype=I16, mdtype=U64)
        info = chain.info()
        assert info["kernel"].startswith("chain_q15pcnd_kernel"), info
        cpws.add(info["tile"])
        idx = out_index(m, nout * D, D)
        same(audio, pairs, r["want"], idx, (D, nout))
        for k in range(meters.shape[0]):          # the meter: the oracle's integer sum over each call's outputs
            lo = k * nout
            for c in range(r["ch"]):
                fi, fq = (r["want"][c][j][idx[lo:lo + nout]].astype(np.int64) for j in (1, 2))
                assert int(meters[k, c]) == int((fi * fi + fq * fq).sum()), (D, nout, k, c)
        chain.close()
    assert len(cpws) >= 2, cpws


def test_one_channel_per_wave_decimated(ctx, dec_ref):
    """a call long enough for one channel per wave (768 outputs at D = 2)"""
    r = dec_ref
    chain = cx_chain(ctx, r["ch"], r["ti"], r["tq"], r["steps"], r["phases"], r["modes"], 0)
    chain.set_decimation(2)
    audio, pairs, _ = cx_run(ctx, chain, r["x"][:, :1536], 1536, 2, pdtype=I16)
    assert chain.info()["tile"] == 512, chain.info()
    same(audio, pairs, r["want"], out_index(1536, 1536, 2), "cpw 1")
    chain.close()


# ------------------------------------------------------------------------------------------------ 5. real input is the special case
@pytest.mark.parametrize("D", [1, 4])
def test_real_input_is_q_zero_dir_one(ctx, golden, D):
    rng = np.random.default_rng(7500 + D)
    ch, n = 10, 512
    modes, ti, tq = bank5(golden, ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=U64)
    x = rng.integers(-30000, 30001, (ch, n)).astype(I16)
    real = nco_chain(ctx, ch, ti, tq, steps, phases, modes)
    cplx = cx_chain(ctx, ch, ti, tq, steps, phases, modes, 1)
    for c in (real, cplx):
        c.set_decimation(D)
    a = cx_run(ctx, real, x, 256, D, pdtype=I16, mdtype=U64)
    b = cx_run(ctx, cplx, interleave(x, np.zeros_like(x)), 256, D, pdtype=I16, mdtype=U64)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    assert np.abs(a[0].astype(np.int32)).max() > 100
    real.close()
    cplx.close()


# ------------------------------------------------------------------------------------------------ 6. one antenna of pairs
def test_ten_receivers_on_one_antenna_row(ctx, orc, golden):
    rng = np.random.default_rng(7600)
    ch, n = 10, 3 * B
    modes, ti, tq = mixed_bank(golden, ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=U64)
    si, sq = Bank(steps, phases).advance(n)
    xi, xq = (rng.integers(-30000, 30001, (1, n)).astype(I16) for _ in range(2))
    chain = cx_chain(ctx, ch, ti, tq, steps, phases, modes, 0)
    chain.set_input_rows(np.zeros(ch, np.int32), 1)
    audio, pairs, _ = cx_run(ctx, chain, interleave(xi, xq), B, ch=ch, pdtype=I16)
    want = refs(orc, np.repeat(xi, ch, 0), np.repeat(xq, ch, 0), si, sq, 0, modes, ti, tq)
    same(audio, pairs, want, np.arange(n), "antenna")
    for c in (0, ch - 1):
        h = chain.fir_history(c)
        assert h.shape[1] == 2 and np.array_equal(h, interleave(xi, xq)[0, n - h.shape[0]:]), c
    chain.close()


# ------------------------------------------------------------------------------------------------ 7. a live retune across a call boundary
def test_a_history_sample_keeps_its_generation(ctx, orc, golden):
    rng = np.random.default_rng(7700)
    ch, n = 4, 512
    modes, ti, tq = mixed_bank(golden, ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=U64)
    new = off_grid_steps(rng, 2)
    bank = Bank(steps, phases)
    s0, c0 = bank.advance(256)
    bank.retune(1, new)
    s1, c1 = bank.advance(256)
    si, sq = np.concatenate([s0, s1], 1), np.concatenate([c0, c1], 1)
    xi, xq = (rng.integers(-30000, 30001, (ch, n)).astype(I16) for _ in range(2))
    x = interleave(xi, xq)
    chain = cx_chain(ctx, ch, ti, tq, steps, phases, modes, 1)
    a0, _, _ = cx_run(ctx, chain, x[:, :256], 256)
    chain.set_nco_channels(1, u32(new))
    a1, _, _ = cx_run(ctx, chain, x[:, 256:], 256)
    bank.check(chain)
    same(np.concatenate([a0, a1], 1), None, refs(orc, xi, xq, si, sq, 1, modes, ti, tq), np.arange(n), "retune")
    chain.close()


# ------------------------------------------------------------------------------------------------ 8. the PLL demodulator behind it
def test_syncam_pll_on_complex_input(ctx, orc, golden):
    rng = np.random.default_rng(7800)
    ch, n = 3, 256
    _, ti, tq = mixed_bank(golden, ch)
    modes = np.array([SYNCAM, SYNCAM, AM], np.int32)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=U64)
    si, sq = Bank(steps, phases).advance(n)
    xi, xq = (rng.integers(-30000, 30001, (ch, n)).astype(I16) for _ in range(2))
    chain = cx_chain(ctx, ch, ti, tq, steps, phases, modes, 0, flags=msdr.CHAIN_SYNCAM_PLL)
    audio, _, _ = cx_run(ctx, chain, interleave(xi, xq), B)
    want = refs(orc, xi, xq, si, sq, 0, modes, ti, tq)
    for c in range(2):
        s = orc.syncam_new()
        pll = np.concatenate([orc.syncam_q15(s, want[c][1][o:o + B], want[c][2][o:o + B]) for o in range(0, n, B)])
        assert np.array_equal(audio[c], pll), c
    assert np.array_equal(audio[2], want[2][0])
    chain.close()


# ------------------------------------------------------------------------------------------------ 9. refusals and state
def test_refusals_and_state(ctx, golden):
    rng = np.random.default_rng(7900)
    ch = 3
    modes, ti, tq = mixed_bank(golden, ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=U64)
    table = msdr.Chain(ctx, msdr.ARITH_Q15, ch, ti[0], tq[0], mixer=msdr.MIXER_NCO, modes=modes, **any_table())
    refused(table.set_complex_input, True, 0)          # not in phase-accumulator mode
    assert table.complex_input() == (False, 0)
    table.close()
    assert ctx.lib.msdr_chain_set_complex_input(None, 1, 0) == ARG and ctx.lib.msdr_chain_get_complex_input(None, None, None) == ARG
    chain = nco_chain(ctx, ch, ti, tq, steps, phases, modes)
    assert chain.complex_input() == (False, 0)
    for bad in (2, -1):
        refused(chain.set_complex_input, True, bad)
        assert chain.complex_input() == (False, 0)
    chain.set_complex_input(False, 7)          # off: dir is not looked at, and nothing changes
    chain.set_complex_input(True, 1)
    x = interleave(*(rng.integers(-30000, 30001, (ch, B)).astype(I16) for _ in range(2)))
    cx_run(ctx, chain, x, B)
    for args in ((False, 0), (True, 0)):          # a switch after a processed call
        refused(chain.set_complex_input, *args)
        assert chain.complex_input() == (True, 1)
    chain.set_complex_input(True, 1)          # the values in force: always accepted
    with pytest.raises(msdr.MsdrError):
        chain.graph([ctx.to_device(x)] * 2, [ctx.array((ch, B), I16)] * 2, B)
    chain.reset()
    assert chain.complex_input() == (True, 1)          # survives reset ...
    chain.set_decimation(2)
    chain.set_meter(None)
    chain.set_iq_out(None)
    assert chain.complex_input() == (True, 1)          # ... and the neighbouring setters
    chain.set_complex_input(True, 0)          # accepted over the cleared history
    chain.set_decimation(1)
    chain.set_nco_channels(0, u32(steps), u32(phases))
    cx_run(ctx, chain, x, B)
    refused(chain.set_complex_input, False, 0)
    chain.init_fir()
    chain.set_complex_input(False, 0)          # and after init_fir
    assert chain.complex_input() == (False, 0)
    h = chain.fir_history(0)
    assert h.ndim == 1 and not h.any()
    chain.close()


def test_nodes_behind_the_complex_mix(ctx, orc, golden):
    """an AudioFilterBiquad node behind the kernel: the composed chain ends in biquad_teensy_update"""
    rng = np.random.default_rng(7950)
    ch, n = 3, 256
    modes, ti, tq = mixed_bank(golden, ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=U64)
    si, sq = Bank(steps, phases).advance(n)
    xi, xq = (rng.integers(-30000, 30001, (ch, n)).astype(I16) for _ in range(2))
    chain = cx_chain(ctx, ch, ti, tq, steps, phases, modes, 0, biquad_nodes=[[lowpass()]])
    audio, _, _ = cx_run(ctx, chain, interleave(xi, xq), B)
    for c, w in enumerate(refs(orc, xi, xq, si, sq, 0, modes, ti, tq)):
        node = orc.biquad_teensy_new([lowpass()])
        assert np.array_equal(audio[c], np.concatenate([orc.biquad_teensy_update(node, w[0][o:o + B]) for o in range(0, n, B)])), c
    chain.close()
