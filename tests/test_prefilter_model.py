"""The expected value of the two-stage chain (tests/prefilter_model.py), without a GPU.

  - With the prefilter that passes the newest sample alone, the fp32 model IS the one-stage chain (cx_cases.compose_f32) with the channel taps
    zero-stuffed by D1, taken at input sample m D1 D2 + D1 D2 - 1: exact zeros are added in the same order, so the two are equal bit for bit.
    The same holds for the Q15 model (cx_cases.compose_q15).
  - For the fp32 inputs of the GPU tests the oracle alone is inside cx_cases.judge_f32's bound e_orc < 2e-6 (fp32 model against float64), per
    channel and per shape: the GPU tests can meet e_go < 1e-5 and e_gpu <= 2 e_orc + 1e-6."""
import numpy as np
import pytest

import cx_cases
import orclib
import prefilter_model as pm
from test_gpu_nco_per_channel import Bank

F = np.float32


@pytest.fixture(scope="module")
def orc():
    return orclib.Oracle()


@pytest.mark.parametrize("D1,D2", [(2, 1), (4, 3), (8, 4)])
def test_the_delta_prefilter_is_the_one_stage_chain_with_zero_stuffed_taps(orc, D1, D2):
    from test_gpu_osc_per_channel_f32 import mixed_bank, signal
    rng = np.random.default_rng([3100, D1, D2])
    ch, n = 4, 96 * D1 * D2
    modes, ti, tq = mixed_bank(ch)
    steps, phases = rng.integers(0, 1 << 32, ch, dtype=np.uint64), rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    x = signal(rng, ch, n)
    si, sq = Bank(steps, phases).advance(n)
    zero = np.zeros(n, np.int16)
    index = np.arange(D1 * D2 - 1, n, D1 * D2)
    for c in range(ch):
        got = pm.model_f32(orc, x[c], si[c], sq[c], pm.delta(D1, F), D1, modes[c], ti[c], tq[c], D2)
        want = cx_cases.compose_f32(orc, x[c], zero, si[c], sq[c], 1, modes[c], pm.zero_stuff(ti[c], D1), pm.zero_stuff(tq[c], D1))
        for g, w in zip(got, want):
            assert np.array_equal(g, w[index]), (c, D1, D2)
        assert np.abs(got[0]).max() > 1e-3


def test_the_q15_delta_prefilter_scales_by_32767_and_nothing_else(orc):
    """Q15: the delta's tap is 32767, not 32768 -- u = (x * 32767) >> 15 -- so the two-stage model is the one-stage chain over THAT stream"""
    rng = np.random.default_rng(3101)
    D1, D2, n = 4, 2, 96 * 8
    t = rng.integers(-2500, 2501, 30).astype(np.int16)
    steps, phases = rng.integers(0, 1 << 32, 1, dtype=np.uint64), rng.integers(0, 1 << 32, 1, dtype=np.uint64)
    x = rng.integers(-30000, 30001, n).astype(np.int16)
    si, sq = Bank(steps, phases).advance(n)
    audio, fi, fq = pm.model_q15(orc, x, si[0], sq[0], pm.delta(D1, np.int16), D1, orclib.LSB, t, t, D2)
    mi, mq = orc.freqconv_q15(x, np.zeros_like(x), si[0], sq[0], 1, 1)
    ui, uq = ((mi.astype(np.int32) * 32767) >> 15).astype(np.int16), ((mq.astype(np.int32) * 32767) >> 15).astype(np.int16)
    index = np.arange(D1 * D2 - 1, n, D1 * D2)
    zs = np.concatenate([np.zeros(1, np.int16), pm.zero_stuff(t, D1)])          # (arm_fir_init_q15 takes even counts: one more zero in front)
    rc, wi = orc.fir_q15_blocks(zs, ui, 128)
    assert rc == 0
    rc, wq = orc.fir_q15_blocks(zs, uq, 128)
    assert rc == 0
    assert np.array_equal(fi, wi[index]) and np.array_equal(fq, wq[index])
    assert np.array_equal(audio, orc.demod_q15(orclib.LSB, wi[index], wq[index]))


@pytest.mark.parametrize("shape", pm.SHAPES)
def test_the_oracle_alone_is_inside_the_judges_bound_for_the_gpu_tests_inputs(orc, shape):
    D1, N1, D2 = shape
    k = pm.case_f32(shape)
    worst = 0.0
    for c in range(k["x"].shape[0]):
        want = pm.model_f32(orc, k["x"][c], k["si"][c], k["sq"][c], k["p"], D1, k["modes"][c], k["ti"][c], k["tq"][c], D2)
        truth = pm.model_f64(k["x"][c], k["si"][c], k["sq"][c], k["p"], D1, k["modes"][c], k["ti"][c], k["tq"][c], D2)
        for name, w, t in zip(("audio", "fi", "fq"), want, truth):
            e = cx_cases.rel(w, t)
            worst = max(worst, e)
            assert e < 2e-6, (shape, c, name, e)
    print("prefilter model %s: worst e_orc %.3e" % (shape, worst))
