"""What the complex-input tests share (msdr_chain_set_complex_input): the expected value composed from the oracle's own stages, and the runner.

Expected value, per receiver, at the full rate:
  freqconv(xi, xq, osc_i = sin, osc_q = cos, dir, 1) -> the FIR pair in blocks of 128 (coeffs_i over I', coeffs_q over Q') -> the demodulator
with the oscillator rows of Bank(steps, phases).advance(n) (tests/test_gpu_nco_per_channel.py).  A decimated output m of a call is the
full-rate value at the call's input m D + D - 1."""
import numpy as np

B = 128
F = np.float32
IN_SCALE = F(1.0 / 32768.0)


def compose_q15(orc, xi, xq, si, sq, direction, mode, ti, tq, sqrt_kind=None):
    """(audio, fi, fq, I', Q') int16 at the full rate for one receiver"""
    mi, mq = orc.freqconv_q15(xi, xq, si, sq, direction, 1)
    rc, fi = orc.fir_q15_blocks(ti, mi, B)
    assert rc == 0
    rc, fq = orc.fir_q15_blocks(tq, mq, B)
    assert rc == 0
    audio = orc.demod_q15(int(mode), fi, fq) if sqrt_kind is None else orc.demod_q15(int(mode), fi, fq, sqrt_kind)
    return audio, fi, fq, mi, mq


def compose_f32(orc, xi, xq, si, sq, direction, mode, ti, tq, in_scale=IN_SCALE):
    """(audio, fi, fq) float32 at the full rate for one receiver: I in_scale, Q in_scale, c / 32768, s / 32768, every operation rounded to fp32"""
    fi_in, fq_in = np.asarray(xi, F) * F(in_scale), np.asarray(xq, F) * F(in_scale)
    oi, oq = (np.asarray(si, np.int16) / 32768.0).astype(F), (np.asarray(sq, np.int16) / 32768.0).astype(F)
    mi, mq = orc.freqconv_f32(fi_in, fq_in, oi, oq, direction, 1)
    fi, fq = orc.fir_f32_blocks(ti, mi, B), orc.fir_f32_blocks(tq, mq, B)
    return orc.demod_f32(int(mode), fi, fq), fi, fq


def compose_f64(xi, xq, si, sq, direction, mode, ti, tq, in_scale=IN_SCALE):
    """the same chain with every operation in float64: (audio, fi, fq)"""
    a, b = np.asarray(xi, np.float64) * float(in_scale), np.asarray(xq, np.float64) * float(in_scale)
    s, c = np.asarray(si, np.float64) / 32768.0, np.asarray(sq, np.float64) / 32768.0
    mi, mq = (a * c - b * s, b * c + a * s) if direction else (a * c + b * s, b * c - a * s)
    n = mi.size
    fi = np.convolve(mi, np.asarray(ti, np.float64)[::-1])[:n]          # CMSIS order: the last coefficient meets the newest sample
    fq = np.convolve(mq, np.asarray(tq, np.float64)[::-1])[:n]
    audio = fi - fq if mode == 2 else fi + fq if mode == 3 else np.sqrt(fi * fi + fq * fq)          # (stations.h:4: LSB 2, USB 3)
    return audio, fi, fq


def rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.sqrt(((got - want) ** 2).sum() / max((want ** 2).sum(), 1e-300)))


def judge_f32(tag, got, want32, truth64):
    """the fp32 chains' contract at level 1, with no excuse: e_go < 1e-5 against the fp32 oracle AND e_gpu <= 2 e_orc + 1e-6 against float64;
    the oracle alone shows that e_go < 1e-5 is within reach (e_orc < 2e-6)"""
    e_go, e_gpu, e_orc = rel(got, want32), rel(got, truth64), rel(want32, truth64)
    print("cx f32 %s e_go %.3e e_gpu %.3e e_orc %.3e" % (tag, e_go, e_gpu, e_orc))
    assert e_orc < 2e-6, (tag, e_orc)
    assert e_go < 1e-5, (tag, e_go)
    assert e_gpu <= 2 * e_orc + 1e-6, (tag, e_gpu, e_orc)


def interleave(xi, xq):
    """[rows, n] and [rows, n] -> [rows, n, 2] int16, the layout of d_if while the mode is on"""
    return np.ascontiguousarray(np.stack([np.asarray(xi, np.int16), np.asarray(xq, np.int16)], axis=-1))


def out_index(n, step, D=1):
    """the full-rate sample behind every output of calls of `step` inputs over the first n"""
    return np.concatenate([np.arange(lo + D - 1, min(lo + step, n), D) for lo in range(0, n, step)])


def pitch_of(n_out):
    return (n_out + 7) // 8 * 8 + 8


def cx_run(ctx, chain, x, step, D=1, ch=None, adtype=np.int16, pdtype=None, mdtype=None):
    """calls of `step` INPUT samples over x ([rows, n, 2] pairs, or [rows, n] on a chain with real input) -> (audio [ch, n / D],
    pairs [ch, n / D, 2] or None, meter [calls, ch] or None).  pdtype: set an I/Q buffer of that type; mdtype: set a meter of that type."""
    n = x.shape[1]
    ch = ch or x.shape[0]
    pitch = pitch_of(min(step, n) // D)
    buf = met = None
    if pdtype is not None:
        buf = ctx.to_device(np.zeros((ch, pitch, 2), pdtype))
        chain.set_iq_out(buf, pitch)
    if mdtype is not None:
        met = ctx.to_device(np.zeros(ch, mdtype))
        chain.set_meter(met)
    audio = np.empty((ch, n // D), adtype)
    pairs = np.empty((ch, n // D, 2), pdtype) if buf is not None else None
    meters = []
    for o in range(0, n, step):
        m = min(step, n - o)
        dx, dy = ctx.to_device(np.ascontiguousarray(x[:, o:o + m])), ctx.array((ch, m // D), adtype)
        chain.process(dx, dy, m)
        audio[:, o // D:(o + m) // D] = dy.download()
        if buf is not None:
            pairs[:, o // D:(o + m) // D] = buf.download()[:, :m // D]
        if met is not None:
            meters.append(met.download().copy())
    return audio, pairs, (np.stack(meters) if met is not None else None)
