"""What the prefilter tests share (msdr_chain_set_prefilter): the expected value of the two-stage chain composed from the oracle's own stages,
a Python statement of the launch rule of minimal-sdr_amd/csrc/msdr_prepc_geometry.h, and the table of tiles the GPU tests hold
msdr_chain_get_info() to (tests/test_prepc_geometry.py holds the table to the header).

Expected value, per receiver, over the whole stream (every call is a multiple of D1 * D2 samples and the chain starts from a clear history, so
the decimation phases of the stream are those of every call):
  the oscillator rows of Bank(steps, phases).advance(n) -> freqconv(x, 0, sin, cos, dir 1, 1): I = x cos, Q = x sin, the real chain's mixer
  -> the prefilter p on both streams, in blocks of 128 -> [D1 - 1 :: D1] -> the channel pair (coeffs_i over u_I, coeffs_q over u_Q) in blocks of
  128 -> [D2 - 1 :: D2] -> the demodulator."""
import numpy as np

B = 128
F = np.float32
IN_SCALE = F(1.0 / 32768.0)
CAP = 64 * 1024
FACTORS = (2, 4, 8, 16, 32)


# ---- the expected value -------------------------------------------------------------------------------------------------------------------------
def model_q15(orc, x, si, sq, p, D1, mode, ti, tq, D2, sqrt_kind=None):
    """(audio, fi, fq) int16 at fs / (D1 D2) for one receiver; p: the prefilter row in CMSIS order (an even count)"""
    x = np.asarray(x, np.int16)
    mi, mq = orc.freqconv_q15(x, np.zeros_like(x), si, sq, 1, 1)
    rc, ui = orc.fir_q15_blocks(p, mi, B)
    assert rc == 0
    rc, uq = orc.fir_q15_blocks(p, mq, B)
    assert rc == 0
    ui, uq = ui[D1 - 1::D1], uq[D1 - 1::D1]
    rc, fi = orc.fir_q15_blocks(ti, ui, B)
    assert rc == 0
    rc, fq = orc.fir_q15_blocks(tq, uq, B)
    assert rc == 0
    fi, fq = fi[D2 - 1::D2], fq[D2 - 1::D2]
    audio = orc.demod_q15(int(mode), fi, fq) if sqrt_kind is None else orc.demod_q15(int(mode), fi, fq, sqrt_kind)
    return audio, fi, fq


def model_f32(orc, x, si, sq, p, D1, mode, ti, tq, D2, in_scale=IN_SCALE):
    """(audio, fi, fq) float32: x in_scale, cos / 32768, sin / 32768, every operation rounded to fp32"""
    xf = np.asarray(x, F) * F(in_scale)
    oi, oq = (np.asarray(si, np.int16) / 32768.0).astype(F), (np.asarray(sq, np.int16) / 32768.0).astype(F)
    mi, mq = orc.freqconv_f32(xf, np.zeros_like(xf), oi, oq, 1, 1)
    ui, uq = orc.fir_f32_blocks(p, mi, B)[D1 - 1::D1], orc.fir_f32_blocks(p, mq, B)[D1 - 1::D1]
    fi, fq = orc.fir_f32_blocks(ti, ui, B)[D2 - 1::D2], orc.fir_f32_blocks(tq, uq, B)[D2 - 1::D2]
    return orc.demod_f32(int(mode), fi, fq), fi, fq


def _fir64(t, x):
    return np.convolve(x, np.asarray(t, np.float64)[::-1])[:x.size]          # CMSIS order: the last coefficient meets the newest sample


def model_f64(x, si, sq, p, D1, mode, ti, tq, D2, in_scale=IN_SCALE):
    """the same chain with every operation in float64: (audio, fi, fq)"""
    a = np.asarray(x, np.float64) * float(in_scale)
    mi, mq = a * (np.asarray(sq, np.float64) / 32768.0), a * (np.asarray(si, np.float64) / 32768.0)
    ui, uq = _fir64(p, mi)[D1 - 1::D1], _fir64(p, mq)[D1 - 1::D1]
    fi, fq = _fir64(ti, ui)[D2 - 1::D2], _fir64(tq, uq)[D2 - 1::D2]
    audio = fi - fq if mode == 2 else fi + fq if mode == 3 else np.sqrt(fi * fi + fq * fq)          # (stations.h:4: LSB 2, USB 3)
    return audio, fi, fq


def zero_stuff(t, D1):
    """the taps t (CMSIS order, designed for fs / D1) as a filter at fs: D1 - 1 zeros between them, the last tap on the newest sample"""
    t = np.asarray(t)
    z = np.zeros((t.size - 1) * D1 + 1, t.dtype)
    z[::D1] = t
    return z


def delta(D1, dtype):
    """the prefilter that passes the newest sample alone: u[j] = mixed[j D1 + D1 - 1]; D1 taps (an even count)"""
    p = np.zeros(D1, dtype)
    p[-1] = 1 if dtype == F else 32767
    return p


def lowpass(D1, nt, dtype):
    """a windowed-sinc anti-alias filter for decimation by D1: unit DC gain, cutoff 0.4 fs / D1"""
    k = np.arange(nt) - (nt - 1) / 2.0
    h = np.sinc(0.8 * k / D1) * np.kaiser(nt, 6.0)
    h /= h.sum()
    return h.astype(F) if dtype == F else np.round(h * 32767.0).astype(np.int16)


# ---- the launch rule, restated --------------------------------------------------------------------------------------------------------------------
def pad(nt, f32):
    q = 4 if f32 else 8
    return (nt + q - 1) // q * q


def chunk(D1, cpw):
    return (64 // cpw) * max(1, 16 // D1)


def hist_len(np1, D1, np2):
    return (np2 - 1) * D1 + np1 - 1


def lds_bytes(f32, np1, D1, np2, D2, cpw, nw, opl):
    tile = opl * (64 // cpw)
    raw = 2 * (chunk(D1, cpw) * D1 + np1)
    if f32:
        per = 4 * (2 * (tile * D2 + np2) + 2 * np2 + raw)
    else:
        per = 2 * (2 * (2 if D2 & 1 else 1) * (tile * D2 + np2) + 2 * np2 + raw)
    return per * cpw * nw + 4096 + np1 * (4 if f32 else 2)


def fits(f32, np1, D1, np2, D2):
    return D1 in FACTORS and np1 > 0 and np2 > 0 and D2 >= 1 and lds_bytes(f32, np1, D1, np2, D2, 1, 1, 2) <= CAP


def geometry(f32, np1, D1, np2, D2, nout, channels, cus, time_segments=0):
    """dict(grid, block, lds_bytes, cpw, nseg, tile, seg_len, nw, opl, chunks) or None: dec_geometry's rule over FINAL outputs"""
    cpw, nw, opl = (4 if nout <= 128 else 2 if nout <= 256 else 1), 4, 8
    size = lambda: lds_bytes(f32, np1, D1, np2, D2, cpw, nw, opl)          # noqa: E731
    while size() > CAP and opl > 2:
        opl //= 2
    while size() > CAP and nw > 1:
        nw //= 2
    while size() > CAP and cpw > 1:
        cpw //= 2
    if size() > CAP or D1 not in FACTORS:
        return None
    tile = opl * (64 // cpw)
    groups, tiles = (channels + cpw - 1) // cpw, (nout + tile - 1) // tile
    nseg = max(1, min((32 * cus + groups - 1) // groups, tiles // 4))
    if time_segments == 1:
        nseg = 1
    elif time_segments > 1:
        nseg = max(1, min(time_segments, tiles))
    seg_tiles = (tiles + nseg - 1) // nseg
    nseg = (tiles + seg_tiles - 1) // seg_tiles
    wlen, C = tile * D2 + np2, chunk(D1, cpw)
    return dict(grid=(groups * nseg + nw - 1) // nw, block=nw * 64, lds_bytes=size(), cpw=cpw, nseg=nseg, tile=tile, seg_len=seg_tiles * tile, nw=nw, opl=opl,
                chunks=(wlen + C - 1) // C)


# ---- what the GPU tests hold msdr_chain_get_info() to -----------------------------------------------------------------------------------------------
# (D1, N1, D2) of the issue's list; 102 channel taps (np2 = 104), 11 channels.  Per arithmetic: the tile in FINAL outputs for calls of 32 / 128 /
# 256 / 768 outputs, written from msdr_prepc_geometry.h (tests/test_prepc_geometry.py runs the header over these shapes).  The window of
# (32, 64, 2) takes 15 .. 20 (Q15) / 6 .. 11 (F32) stage-1 chunks per tile, that of (8, 32, 4) 12 .. 18 / 5 .. 8; SEGMENTED is the one call of
# 4096 outputs at (4, 16, 4) that runs in more than one time segment (on 256 compute units).
SHAPES = ((2, 8, 1), (2, 30, 3), (4, 16, 4), (8, 32, 4), (32, 64, 2))
NOUTS = (32, 128, 256, 768)
NT2, CH = 102, 11
TILES = {
    "q15": {(2, 8, 1): (128, 128, 256, 512), (2, 30, 3): (32, 32, 128, 256), (4, 16, 4): (64, 64, 256, 512), (8, 32, 4): (64, 64, 256, 512),
            (32, 64, 2): (64, 64, 256, 512)},
    "f32": {(2, 8, 1): (32, 32, 128, 512), (2, 30, 3): (32, 32, 64, 128), (4, 16, 4): (32, 32, 64, 128), (8, 32, 4): (32, 32, 64, 128),
            (32, 64, 2): (32, 32, 64, 128)},
}
MIN_CHUNKS = {"q15": {(32, 64, 2): 15, (8, 32, 4): 12}, "f32": {(32, 64, 2): 6, (8, 32, 4): 5}}
SEGMENTED = dict(shape=(4, 16, 4), nout=4096, tile={"q15": 512, "f32": 128}, nseg={"q15": 2, "f32": 8})


# ---- the inputs of the fp32 GPU tests (tests/test_prefilter_model.py holds the oracle alone to judge_f32's e_orc bound over them) -------------------
def step_list(rng):
    """0, 5 * 2^25, fs / 4, -fs / 4, one LSB below zero and six seeded ones"""
    return np.concatenate([np.array([0, 5 << 25, 0x40000000, 0xC0000000, 0xFFFFFFFF], np.uint64), rng.integers(0, 1 << 32, 6, dtype=np.uint64)])


def case_f32(shape, nout=768):
    """dict(x, steps, phases, modes, ti, tq, p, si, sq) of the fp32 geometry case of `shape`: 11 channels, AM / LSB / USB / CW, 102 taps"""
    from test_gpu_nco_per_channel import Bank
    from test_gpu_osc_per_channel_f32 import mixed_bank, signal
    D1, N1, D2 = shape
    rng = np.random.default_rng([3300, D1, N1, D2])
    steps = step_list(rng)
    ch = steps.size
    modes, ti, tq = mixed_bank(ch)
    phases = rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    n = nout * D1 * D2
    x = signal(rng, ch, n)
    si, sq = Bank(steps, phases).advance(n)
    return dict(x=x, steps=steps, phases=phases, modes=modes, ti=ti, tq=tq, p=lowpass(D1, N1, F), si=si, sq=sq)
