"""Complex I/Q input of the per-receiver down-converter bank (F32): msdr_chain_set_complex_input on fp32 chains.

Expected value: tests/cx_cases.py's composed fp32 oracle (freqconv_f32 -> fir_f32_blocks pair -> demod_f32).  Judged per channel as the fp32
chains are (tests/f32judge.py at level 1, cx_cases.judge_f32): e_go < 1e-5 against the fp32 oracle and e_gpu <= 2 e_orc + 1e-6 against the same
chain in float64, no channel excused; pairs are held to the same 1e-5.  Every figure is printed."""
import numpy as np
import pytest

from cx_cases import B, compose_f32, compose_f64, cx_run, interleave, judge_f32, out_index
from gpuhelp import ctx, msdr  # noqa: F401
from test_gpu_decim_per_channel import step_list
from test_gpu_decim_per_channel_f32 import nco_chain
from test_gpu_nco_per_channel import Bank, off_grid_steps
from test_gpu_osc_per_channel_f32 import mixed_bank, signal

pytestmark = pytest.mark.gpu
F, F64, U64 = np.float32, np.float64, np.uint64
CX = msdr.FLAVOUR_COMPLEX_IN


def cx_chain(ctx, ch, ti, tq, steps, phases, modes, direction, **kw):
    chain = nco_chain(ctx, ch, ti, tq, steps, phases, modes=modes, **kw)
    chain.set_complex_input(True, direction)
    return chain


def refs(orc, xi, xq, si, sq, direction, modes, ti, tq):
    return [(compose_f32(orc, xi[c], xq[c], si[c], sq[c], direction, modes[c], ti[c], tq[c]),
             compose_f64(xi[c], xq[c], si[c], sq[c], direction, modes[c], ti[c], tq[c])) for c in range(len(modes))]


def judged(tag, audio, pairs, want, idx):
    for c, (w32, w64) in enumerate(want):
        judge_f32("%s ch %d" % (tag, c), audio[c], w32[0][idx], w64[0][idx])
        if pairs is not None:
            p, i, q = pairs[c].astype(F64), w32[1][idx].astype(F64), w32[2][idx].astype(F64)
            ratio = float(np.sqrt(((p[:, 0] - i) ** 2 + (p[:, 1] - q) ** 2).sum()) / np.sqrt((i * i + q * q).sum()))
            print("cx f32 %s ch %d pairs %.3e" % (tag, c, ratio))
            assert ratio < 1e-5, (tag, c, ratio)


# ------------------------------------------------------------------------------------------------ 1. every sliding-window geometry
@pytest.mark.parametrize("direction", [0, 1])
def test_every_sliding_window_geometry(ctx, orc, direction):
    rng = np.random.default_rng(8100 + direction)
    ch, n = 10, 6 * B
    modes, ti, tq = mixed_bank(ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=U64)
    si, sq = Bank(steps, phases).advance(n)
    xi, xq = signal(rng, ch, n), signal(rng, ch, n)
    want = refs(orc, xi, xq, si, sq, direction, modes, ti, tq)
    runs = []
    for step, tile in ((B, 128), (2 * B, 256), (n, 512)):
        chain = cx_chain(ctx, ch, ti, tq, steps, phases, modes, direction)
        audio, pairs, _ = cx_run(ctx, chain, interleave(xi, xq), step, adtype=F, pdtype=F)
        info = chain.info()
        assert info["kernel"].startswith("chain_f32pcn_kernel") and info["tile"] == tile and info["flavour"] & CX, info
        judged("dir %d step %d" % (direction, step), audio, pairs, want, np.arange(n))
        runs.append((audio, pairs))
        chain.close()
    for a, p in runs[1:]:          # (a lane's sums do not depend on the tile)
        assert np.array_equal(a.view(np.uint32), runs[0][0].view(np.uint32)) and np.array_equal(p.view(np.uint32), runs[0][1].view(np.uint32))


# ------------------------------------------------------------------------------------------------ 3. the tail and the segments
@pytest.mark.parametrize("n, segs", [(1001, 0), (4600, 0), (4600, 3)])
def test_the_tail_and_the_segments(ctx, orc, n, segs):
    rng = np.random.default_rng(8300 + n + segs)
    ch = 3
    modes, ti, tq = mixed_bank(ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=U64)
    si, sq = Bank(steps, phases).advance(n)
    xi, xq = signal(rng, ch, n), signal(rng, ch, n)
    chain = cx_chain(ctx, ch, ti, tq, steps, phases, modes, 0, time_segments=segs)
    audio, pairs, _ = cx_run(ctx, chain, interleave(xi, xq), n, adtype=F, pdtype=F)
    info = chain.info()
    assert info["tile"] == 512 and info["time_segments"] == (1 if n == 1001 else segs or 2), info
    judged("n %d segs %d" % (n, segs), audio, pairs, refs(orc, xi, xq, si, sq, 0, modes, ti, tq), np.arange(n))
    chain.close()


# ------------------------------------------------------------------------------------------------ 4. decimation
@pytest.fixture(scope="module")
def dec_ref(orc):
    rng = np.random.default_rng(8400)
    steps = step_list(rng)
    ch = steps.size
    modes, ti, tq = mixed_bank(ch)
    phases = rng.integers(0, 1 << 32, ch, dtype=U64)
    n = 301 * 8
    xi, xq = signal(rng, ch, n), signal(rng, ch, n)
    si, sq = Bank(steps, phases).advance(n)
    return dict(steps=steps, phases=phases, modes=modes, ti=ti, tq=tq, x=interleave(xi, xq), want=refs(orc, xi, xq, si, sq, 0, modes, ti, tq), ch=ch)


@pytest.mark.parametrize("D", [3, 2, 8])
def test_decimation(ctx, dec_ref, D):
    """D = 3, 2, 8: read widths AL 1, 2, 4.  256 D inputs in calls of 32 and 128 outputs and one of 256 (4 / 4 / 2 channels per wave), one call
    of 301 outputs (a partial last tile); meter and I/Q buffer both set.  The meter: within tests/test_gpu_meter_per_channel_f32.py's tolerance
    (2.5e-5 relative) of the oracle's sum of squares"""
    r = dec_ref
    tiles = set()
    for nout in (32, 128, 256, 301):
        chain = cx_chain(ctx, r["ch"], r["ti"], r["tq"], r["steps"], r["phases"], r["modes"], 0)
        chain.set_decimation(D)
        m = (301 if nout == 301 else 256) * D
        audio, pairs, meters = cx_run(ctx, chain, r["x"][:, :m], nout * D, D, adtype=F, pdtype=F, mdtype=F64)
        info = chain.info()
        assert info["kernel"].startswith("chain_f32pcnd_kernel") and info["flavour"] & CX and info["flavour"] & msdr.FLAVOUR_DECIMATED, info
        tiles.add(info["tile"])
        idx = out_index(m, nout * D, D)
        judged("D %d nout %d" % (D, nout), audio, pairs, r["want"], idx)
        for k in range(meters.shape[0]):
            lo = k * nout
            for c in range(r["ch"]):
                fi, fq = (r["want"][c][0][j][idx[lo:lo + nout]].astype(F64) for j in (1, 2))
                want = float((fi * fi + fq * fq).sum())
                print("cx f32 meter D %d nout %d call %d ch %d rel %.3e" % (D, nout, k, c, abs(meters[k, c] - want) / want))
                assert abs(meters[k, c] - want) <= 2.5e-5 * want, (D, nout, k, c)
        chain.close()
    assert len(tiles) >= 2, tiles


def test_one_channel_per_wave_decimated(ctx, dec_ref):
    r = dec_ref
    chain = cx_chain(ctx, r["ch"], r["ti"], r["tq"], r["steps"], r["phases"], r["modes"], 0)
    chain.set_decimation(2)
    audio, pairs, _ = cx_run(ctx, chain, r["x"][:, :1536], 1536, 2, adtype=F, pdtype=F)
    assert chain.info()["tile"] == 512, chain.info()
    judged("cpw 1", audio, pairs, r["want"], out_index(1536, 1536, 2))
    chain.close()


# ------------------------------------------------------------------------------------------------ 5. real input is the special case
@pytest.mark.parametrize("D", [1, 4])
def test_real_input_is_q_zero_dir_one(ctx, D):
    rng = np.random.default_rng(8500 + D)
    ch, n = 10, 512
    modes, ti, tq = mixed_bank(ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=U64)
    x = signal(rng, ch, n)
    real = nco_chain(ctx, ch, ti, tq, steps, phases, modes=modes)
    cplx = cx_chain(ctx, ch, ti, tq, steps, phases, modes, 1)
    for c in (real, cplx):
        c.set_decimation(D)
    a = cx_run(ctx, real, x, 256, D, adtype=F, pdtype=F, mdtype=F64)
    b = cx_run(ctx, cplx, interleave(x, np.zeros_like(x)), 256, D, adtype=F, pdtype=F, mdtype=F64)
    for u, v in zip(a, b):
        assert np.array_equal(u, v)          # equal as values (a zero may differ in sign)
    assert not real.info()["flavour"] & CX and cplx.info()["flavour"] == real.info()["flavour"] | CX
    real.close()
    cplx.close()


# ------------------------------------------------------------------------------------------------ 6. one antenna of pairs
def test_ten_receivers_on_one_antenna_row(ctx, orc):
    rng = np.random.default_rng(8600)
    ch, n = 10, 3 * B
    modes, ti, tq = mixed_bank(ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=U64)
    si, sq = Bank(steps, phases).advance(n)
    xi, xq = signal(rng, 1, n), signal(rng, 1, n)
    chain = cx_chain(ctx, ch, ti, tq, steps, phases, modes, 0)
    for _ in range(2):
        chain.set_input_rows(np.zeros(ch, np.int32), 1)
    audio, pairs, _ = cx_run(ctx, chain, interleave(xi, xq), B, ch=ch, adtype=F, pdtype=F)
    judged("antenna", audio, pairs, refs(orc, np.repeat(xi, ch, 0), np.repeat(xq, ch, 0), si, sq, 0, modes, ti, tq), np.arange(n))
    h = chain.fir_history(ch - 1)
    assert h.shape[1] == 2 and np.array_equal(h, interleave(xi, xq)[0, n - h.shape[0]:])
    chain.close()


# ------------------------------------------------------------------------------------------------ int16 output, the flavour bit, the refusals
def test_int16_output_within_one_lsb(ctx, orc):
    rng = np.random.default_rng(8700)
    ch, n = 4, 2 * B
    modes, ti, tq = mixed_bank(ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=U64)
    si, sq = Bank(steps, phases).advance(n)
    xi, xq = signal(rng, ch, n), signal(rng, ch, n)
    chain = cx_chain(ctx, ch, ti, tq, steps, phases, modes, 0, flags=msdr.CHAIN_OUT_I16)
    audio, _, _ = cx_run(ctx, chain, interleave(xi, xq), B, adtype=np.int16)
    for c, (w32, _) in enumerate(refs(orc, xi, xq, si, sq, 0, modes, ti, tq)):
        want = np.clip(np.round(w32[0].astype(F64) * 32768.0), -32768, 32767)
        assert np.abs(audio[c].astype(F64) - want).max() <= 1, c
    chain.close()


def test_the_flavour_bit_exactly_while_on_and_the_refusals(ctx):
    rng = np.random.default_rng(8800)
    ch = 3
    modes, ti, tq = mixed_bank(ch)
    steps, phases = off_grid_steps(rng, ch), rng.integers(0, 1 << 32, ch, dtype=U64)
    chain = nco_chain(ctx, ch, ti, tq, steps, phases, modes=modes)
    x = signal(rng, ch, B)
    cx_run(ctx, chain, x, B, adtype=F)
    assert not chain.info()["flavour"] & CX
    with pytest.raises(msdr.MsdrError) as e:
        chain.set_complex_input(True, 0)          # a processed call lies in the history
    assert e.value.status == msdr.STATUS_ARGUMENT_ERROR and chain.complex_input() == (False, 0)
    chain.reset()
    chain.set_complex_input(True, 0)
    cx_run(ctx, chain, interleave(x, x), B, adtype=F)
    assert chain.info()["flavour"] & CX
    chain.init_fir()
    chain.set_complex_input(False, 0)
    cx_run(ctx, chain, x, B, adtype=F)
    assert not chain.info()["flavour"] & CX
    chain.close()
