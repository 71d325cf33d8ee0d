"""tests/pll_model.py pinned to the oracle: at the reference's constants the model's audio and state equal orc_syncam_q15's and
orc_syncam_f32's bit for bit, over 22 500 steps that take the loop through lock-in (a carrier 60 Hz off), both omega2 clamps and both
phase wraps (glides to a carrier 5 kHz off, above and then below).  That the inputs reach all four branches is checked on the model's own counters.
No GPU needed."""
import numpy as np

import pll_model

FS = 24000.0
SEG = 1500


def carrier():
    """I + jQ = A exp(j phase): a carrier 60 Hz off (lock-in), a glide the locked loop follows up to its limit and a carrier 5 kHz off above
    it, the glide down through zero to the other limit and the carrier 5 kHz off below; the phase runs on through the joints"""
    f = np.concatenate([np.full(SEG, 60.0), np.linspace(60.0, 4400.0, 4 * SEG), np.full(SEG, 5000.0), np.linspace(4400.0, -4400.0, 8 * SEG),
                        np.full(SEG, -5000.0)])
    ph = 2 * np.pi * np.cumsum(f) / FS + 0.4
    return np.cos(ph), np.sin(ph)


def test_the_constants_are_the_oracles(orc):
    k = pll_model.constants_f64(FS).astype(np.float32)
    assert np.array_equal(k.view(np.uint32), orc.syncam_constants().view(np.uint32)), (k, orc.syncam_constants())


def test_q15_audio_and_state_equal_the_oracle_through_every_branch(orc):
    c, s = carrier()
    i, q = np.round(9000 * c).astype(np.int16), np.round(9000 * s).astype(np.int16)
    assert i.size >= 4000
    m = pll_model.Pll(orc.syncam_constants())
    st = orc.syncam_new()
    got, want = np.empty(i.size, np.int16), np.empty(i.size, np.int16)
    cuts = (0, 200, 208, SEG, 3 * SEG - 7, i.size)          # (the state carried over calls of several lengths)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        got[lo:hi] = m.run_q15(i[lo:hi], q[lo:hi])
        want[lo:hi] = orc.syncam_q15(st, i[lo:hi], q[lo:hi])
        assert np.array_equal(m.state().view(np.uint32), np.array([st.fil_out, st.omega2, st.phzerror], np.float32).view(np.uint32)), hi
    assert np.array_equal(got, want)
    assert all(v > 0 for v in m.hits.values()), m.hits
    # lock-in: behind 1 000 samples of the 60 Hz carrier the audio is the carrier's amplitude
    assert np.abs(got[1000:SEG].astype(np.int32) - 9000).max() < 200, np.abs(got[1000:SEG].astype(np.int32) - 9000).max()


def test_f32_audio_and_state_equal_the_oracle_through_every_branch(orc):
    c, s = carrier()
    i, q = (0.27 * c).astype(np.float32), (0.27 * s).astype(np.float32)
    m = pll_model.Pll(orc.syncam_constants())
    st = orc.syncam_new()
    got, want = m.run_f32(i, q), orc.syncam_f32(st, i, q)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(m.state().view(np.uint32), np.array([st.fil_out, st.omega2, st.phzerror], np.float32).view(np.uint32))
    assert all(v > 0 for v in m.hits.values()), m.hits
