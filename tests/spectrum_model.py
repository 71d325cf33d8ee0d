"""A numpy model of msdr_chain_set_spectrum's host rules and of the transform's layouts (tests/test_spectrum_model.py holds it against the
oracle; the GPU tests hold the library against it).

  Tick    showSpectrum's cadence (UI.cpp:534-535): `if (--counter > 0) no spectrum; else counter = every, draw`, the counter starting at 0
  Tail    the window: after every call the last 64 of (old tail ++ the call's pairs), per receiver
  cfft64_q15   arm_cfft_q15 of length 64, forward, with bit reversal: what orc.rfft128_q15 leaves in `work`, read as 64 pairs
  cfft64_f64   float64 fft / 64 of the same pairs
  display      bins' power in display order: column x = re^2 + im^2 of bin (x + 32) & 63"""
import numpy as np

BINS = 64


class Tick:
    def __init__(self, every=0):
        self.every, self.counter, self.drawn = every, 0, 0

    def tick(self):
        self.counter -= 1
        if self.counter > 0:
            return False
        self.counter = self.every if self.every else 25
        self.drawn += 1
        return True

    def reset(self):
        self.counter = 0


class Tail:
    def __init__(self, channels, dtype=np.int16):
        self.w = np.zeros((channels, BINS, 2), dtype)

    def push(self, pairs):
        """pairs [channels, n, 2] of one call -> the window [channels, 64, 2] behind it"""
        pairs = np.asarray(pairs)
        assert pairs.shape[0] == self.w.shape[0] and pairs.shape[2] == 2
        self.w = np.concatenate([self.w, pairs.astype(self.w.dtype)], axis=1)[:, -BINS:]
        return self.w

    def clear(self):
        self.w[...] = 0


def cfft64_q15(orc, pairs):
    """[64, 2] int16 -> bins [64, 2] int16, natural order"""
    row = np.ascontiguousarray(pairs, np.int16).reshape(2 * BINS)
    return orc.rfft128_q15(row)[1].reshape(BINS, 2).copy()


def cfft64_f64(pairs):
    """[64, 2] -> complex128 [64]: (1 / 64) sum_m z[m] exp(-2 pi i k m / 64)"""
    p = np.asarray(pairs, np.float64)
    return np.fft.fft(p[:, 0] + 1j * p[:, 1]) / BINS


def display(power):
    """[..., 64] in bin order -> display order"""
    return np.roll(power, BINS // 2, axis=-1)


def power_q15(bins):
    """[64, 2] int16 -> the exact re^2 + im^2 in display order, int64"""
    b = np.asarray(bins).astype(np.int64)
    return display(b[..., 0] ** 2 + b[..., 1] ** 2)


def tone(k, amp=16384, phase=0.0):
    """a complex tone of amplitude amp on bin k: [64, 2] int16"""
    m = np.arange(BINS)
    z = amp * np.exp(1j * (2 * np.pi * k * m / BINS + phase))
    return np.stack([np.round(z.real), np.round(z.imag)], axis=1).astype(np.int16)


def stage_rows(rng):
    """the row set of the stage tests: name -> [64, 2] int16"""
    alt = np.where(np.arange(BINS) % 2 == 0, -32768, 32767)
    rows = {
        "random": rng.integers(-32768, 32768, (BINS, 2)),
        "random2": rng.integers(-32768, 32768, (BINS, 2)),
        "all_min": np.full((BINS, 2), -32768),
        "all_max": np.full((BINS, 2), 32767),
        "alt_per_sample": np.tile(np.array([-32768, 32767]), (BINS, 1)),
        "alt_per_pair": np.stack([alt, alt], axis=1),
        "impulse0": np.zeros((BINS, 2)),
        "impulse63": np.zeros((BINS, 2)),
    }
    rows["impulse0"][0] = (32767, -32768)
    rows["impulse63"][63] = (-32768, 32767)
    for k in (0, 5, 32, 59):
        rows["tone%d" % k] = tone(k)
    return {n: np.asarray(r).astype(np.int16) for n, r in rows.items()}
