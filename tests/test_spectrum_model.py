"""tests/spectrum_model.py against the oracle: showSpectrum's cadence, the window rule, and the Q15 transform's sign, order and scale.  CPU only."""
import ctypes as C

import numpy as np

import spectrum_model as M


def test_the_tick_sequence_is_the_oracles(orc):
    cnt = C.c_int(0)
    want = [bool(orc.lib.orc_spectrum_tick(1, C.byref(cnt))) for _ in range(100)]
    t = M.Tick(25)
    got = [t.tick() for _ in range(100)]
    assert got == want and [i for i, g in enumerate(got) if g] == [0, 25, 50, 75] and t.drawn == 4
    t0 = M.Tick(0)
    assert [t0.tick() for _ in range(100)] == want          # every = 0 means 25
    t1, t3 = M.Tick(1), M.Tick(3)
    assert all(t1.tick() for _ in range(10))
    assert [i for i in range(8) if t3.tick()] == [0, 3, 6]


def test_the_tail_is_the_last_64_of_the_concatenation():
    rng = np.random.default_rng(1)
    ch = 3
    tail, seen = M.Tail(ch), np.zeros((ch, M.BINS, 2), np.int16)
    for n in (16, 16, 24, 64, 1, 130):
        p = rng.integers(-32768, 32768, (ch, n, 2)).astype(np.int16)
        seen = np.concatenate([seen, p], axis=1)
        assert np.array_equal(tail.push(p), seen[:, -M.BINS:]), n
    tail.clear()
    assert not tail.w.any()


def test_a_tone_lands_in_its_bin_forward_sign_scale_one_64th(orc):
    for k in (0, 5, 32, 59):
        bins = M.cfft64_q15(orc, M.tone(k)).astype(np.int64)
        assert np.abs(bins[k]).max() >= 16000, (k, bins[k])
        others = np.delete(bins, k, axis=0)
        assert np.abs(others).max() <= 16, (k, np.abs(others).max())
    bins = M.cfft64_q15(orc, M.tone(5))
    assert bins[5].tolist() == [16382, -1]
    ref = M.cfft64_f64(M.tone(5))
    dev = np.abs(np.stack([ref.real, ref.imag], axis=1) - bins).max()
    assert dev <= 3.0, dev          # 2.9: three truncating stages
    assert M.power_q15(bins).argmax() == 5 + 32          # display order: column 32 is the tuned frequency


def test_the_extreme_row_fills_bin_0_and_a_uint32(orc):
    bins = M.cfft64_q15(orc, np.full((64, 2), -32768, np.int16))
    assert bins[0].tolist() == [-32768, -32768] and not bins[1:].any()
    p = M.power_q15(bins)
    assert p[32] == 2 ** 31 and p.sum() == 2 ** 31 and p.max() < 2 ** 32
