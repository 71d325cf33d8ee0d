"""A Python model of the synchronous-AM PLL (Minimal-SDR.ino:631-688) with the loop constants as a PARAMETER -- what the oracle's
orc_syncam_q15 / orc_syncam_f32 compute with the reference's constants built in, for the bank that runs its loop at fs / D with
msdr_syncam_constants_rate(fs / D) (msdr_chain_set_pll_rate).  Every float operation is one numpy.float32 operation, sin / cos / atan2 are
math's doubles rounded once, as the oracle and the kernels evaluate them.  tests/test_pll_model.py pins it to the oracle at the reference's
constants (audio and state, bit for bit); tests/agc_model.py has the same role for the AGC.  Not collected by pytest."""
import math

import numpy as np

F = np.float32
TWO_PI = 2.0 * 3.1415926535897932384626433832795


def constants_f64(sample_rate):
    """the four initialisers (Minimal-SDR.ino:636-641) under C's arithmetic conversions with SAMPLE_RATE replaced, every libm call in float64:
    omegaN and zeta are floats, so the subexpressions that hold only them and the rate are float products, everything that meets a double
    literal is double.  -> float64 [omega_min, omega_max, g1, g2] BEFORE the final rounding to float (g2: from the rounded g1)"""
    omegaN, zeta = F(400.0), F(0.45)
    fs = float(sample_rate)
    omega_min = 2.0 * math.pi * -4000.0 / fs
    omega_max = 2.0 * math.pi * 4000.0 / fs
    g1 = 1.0 - math.exp(-2.0 * float(omegaN) * float(zeta) / fs)
    e_arg = F(-omegaN * zeta) / F(fs)
    root = F(math.sqrt(float(F(1.0 - float(zeta * zeta)))))
    c_arg = F(F(omegaN / F(fs)) * root)
    g2 = -float(F(g1)) + 2.0 * (1.0 - math.exp(float(e_arg)) * float(F(math.cos(float(c_arg)))))
    return np.array([omega_min, omega_max, g1, g2], np.float64)


class Pll:
    """one channel's loop: state fil_out, omega2, phzerror (float32), constants k = (omega_min, omega_max, g1, g2)"""

    def __init__(self, k):
        self.k = [F(v) for v in k]
        self.fil_out, self.omega2, self.phz = F(0.0), F(0.0), F(0.0)
        self.hits = dict(clamp_min=0, clamp_max=0, wrap_up=0, wrap_down=0)

    def state(self):
        return np.array([self.fil_out, self.omega2, self.phz], np.float32)

    def step(self, fi, fq):
        """fi, fq: float32 -> corr[0] as float32"""
        omega_min, omega_max, g1, g2 = self.k
        Sin, Cos = F(math.sin(float(self.phz))), F(math.cos(float(self.phz)))
        ai, bi = F(Cos * fi), F(Sin * fi)
        aq, bq = F(Cos * fq), F(Sin * fq)
        corr0, corr1 = F(ai + bq), F(-bi + aq)
        det = F(math.atan2(float(corr1), float(corr0)))
        del_out = self.fil_out
        self.omega2 = F(self.omega2 + F(g2 * det))
        if self.omega2 < omega_min:
            self.omega2 = omega_min
            self.hits["clamp_min"] += 1
        elif self.omega2 > omega_max:
            self.omega2 = omega_max
            self.hits["clamp_max"] += 1
        self.fil_out = F(F(g1 * det) + self.omega2)
        self.phz = F(self.phz + del_out)
        while float(self.phz) >= TWO_PI:
            self.phz = F(float(self.phz) - TWO_PI)
            self.hits["wrap_up"] += 1
        while float(self.phz) < 0.0:
            self.phz = F(float(self.phz) + TWO_PI)
            self.hits["wrap_down"] += 1
        return corr0

    def run_q15(self, i, q):
        """int16 I, Q -> int16 audio: (int16)(int32) corr[0], wrapping"""
        out = np.empty(len(i), np.int16)
        for n in range(len(i)):
            c = self.step(F(int(i[n])), F(int(q[n])))
            out[n] = np.int32(int(c)).astype(np.int16) if -2147483648.0 <= float(c) < 2147483648.0 else 0
        return out

    def run_f32(self, i, q):
        out = np.empty(len(i), np.float32)
        for n in range(len(i)):
            out[n] = self.step(F(i[n]), F(q[n]))
        return out
