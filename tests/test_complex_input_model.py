"""The complex-input tests' own model (tests/cx_cases.py) against the oracle's chain: with xq = 0 and dir = 1 the composed reference --
freqconv -> FIR pair -> demodulator -- IS orc.chain_q15(mixer = 1) / orc.chain_f32, and on a full-scale input the two directions differ and
the second saturation of freq_conv (that of the sum) is met.  CPU only."""
import numpy as np
import pytest

import orclib
from cx_cases import B, compose_f32, compose_f64, compose_q15, rel

AM, LSB, USB, CW = orclib.AM, orclib.LSB, orclib.USB, orclib.CW


def osc_rows(rng, n):
    """(sin, cos) int16 rows of a phase that moves by an odd step per sample"""
    ph = 2 * np.pi * ((rng.integers(0, 1 << 32) + np.arange(n) * (int(rng.integers(0, 1 << 32)) | 1)) % (1 << 32)) / float(1 << 32)
    return np.round(32767 * np.sin(ph)).astype(np.int16), np.round(32767 * np.cos(ph)).astype(np.int16)


@pytest.mark.parametrize("mode", [AM, LSB, USB, CW])
def test_q_zero_dir_one_is_the_oracles_q15_chain(orc, golden, mode):
    rng = np.random.default_rng(900 + mode)
    n = 3 * B
    ti, tq = (np.asarray(golden["taps/FIR_SSB_%s_coeffs" % k], np.int16) for k in "IQ")
    x = rng.integers(-30000, 30001, n).astype(np.int16)
    si, sq = osc_rows(rng, n)
    audio, fi, fq, _, _ = compose_q15(orc, x, np.zeros_like(x), si, sq, 1, mode, ti, tq)
    state, want = {}, []
    for o in range(0, n, B):
        want.append(orc.chain_q15(x[o:o + B], mode, ti, tq, mixer=1, osc_i=si[o:o + B], osc_q=sq[o:o + B], state=state, want_iq=True))
    wa, wi, wq = (np.concatenate(p) for p in zip(*want))
    assert np.array_equal(audio, wa) and np.array_equal(fi, wi) and np.array_equal(fq, wq)
    assert np.abs(wa.astype(np.int32)).max() > 100


@pytest.mark.parametrize("mode", [AM, LSB, USB])
def test_q_zero_dir_one_is_the_oracles_f32_chain(orc, mode):
    rng = np.random.default_rng(950 + mode)
    n = B
    k = np.arange(100)
    proto = np.sinc(1920 / 24000 * (k - 49.5)) * np.kaiser(100, 6.0)
    proto /= proto.sum()
    hi = (2 * proto * np.cos(2 * np.pi * 1330 / 24000 * (k - 49.5) + np.pi / 4)).astype(np.float32)
    hq = (2 * proto * np.cos(2 * np.pi * 1330 / 24000 * (k - 49.5) - np.pi / 4)).astype(np.float32)
    x = rng.integers(-20000, 20001, n).astype(np.int16)
    si, sq = osc_rows(rng, n)
    audio, _, _ = compose_f32(orc, x, np.zeros_like(x), si, sq, 1, mode, hi, hq)
    want = orc.chain_f32(x, mode, hi, hq, (si / 32768.0).astype(np.float32), (sq / 32768.0).astype(np.float32), None)
    assert np.array_equal(audio, want)
    assert rel(audio, compose_f64(x, np.zeros_like(x), si, sq, 1, mode, hi, hq)[0]) < 2e-6          # the float64 twin of the model agrees


def test_full_scale_input_the_directions_differ_and_a_sum_saturates(orc, golden):
    rng = np.random.default_rng(990)
    n = 2 * B
    ti, tq = (np.asarray(golden["taps/FIR_SSB_%s_coeffs" % k], np.int16) for k in "IQ")
    xi, xq = (rng.choice(np.array([-32768, 32767], np.int16), n) for _ in range(2))
    ph = 2 * np.pi * (0.125 + 1e-4 * np.arange(n))          # near 45 degrees: c ~ s
    si, sq = np.round(32767 * np.sin(ph)).astype(np.int16), np.round(32767 * np.cos(ph)).astype(np.int16)
    d0, d1 = (compose_q15(orc, xi, xq, si, sq, d, LSB, ti, tq) for d in (0, 1))
    assert not np.array_equal(d0[0], d1[0]) and not np.array_equal(d0[3], d1[3])
    sat = lambda v: np.clip(v, -32768, 32767)          # noqa: E731
    p = lambda a, b: sat((a.astype(np.int64) * b.astype(np.int64)) >> 15)          # noqa: E731
    for d, got in ((0, d0), (1, d1)):
        raw = p(xi, sq) + (-1 if d else 1) * p(xq, si)
        assert ((raw > 32767) | (raw < -32768)).any(), d
        assert np.array_equal(got[3], sat(raw).astype(np.int16)), d          # I' of the oracle is the saturated sum of saturated products
        assert np.isin(got[3], (32767, -32768)).any(), d
