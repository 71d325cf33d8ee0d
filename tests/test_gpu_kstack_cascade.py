"""The folded cascade's two sparse matrix products, R sigma (the state a row starts from) and Rd delta (the previous row's last inputs), with
their split-fp16 terms stacked along K (minimal-sdr_amd/csrc/msdr_kstack.h): every kernel flavour that issues them, at the places where a wrong
sigma or delta operand shows -- row, tile and call boundaries -- held to BOTH clauses of the fp32 contract (tests/f32judge.py) exactly as
tests/test_gpu_f32_flavours.py holds its census: within 1e-5 of the fp32 oracle and within 2 e_orc + fp32_noise + 1e-6 of float64.

Wave-stream cases: 3 channels (the workgroup has idle waves), a call of 2 x 1024 + 32 + 5 samples continued by one of 1024 + 77: the state
hand-off falls mid-row.  Block cadence: 33 channels x 128 samples x 5 ticks.  Every case asserts through info() that the flavour it means
to test is the one that ran.

The case with time_segments=2 at n = 4096 + 37: the host never splits a call of five tiles (a segment is at least four tiles and 32 warm-up
tiles long, msdr_chain_process), so that call runs as ONE segment -- the case stays as it is and says so; "segmented_64k" is the
same configuration at the shortest length the host does split in two (64 tiles + 37), judged around the boundary as the census judges."""
import numpy as np
import pytest

import orclib
from f32judge import fp32_noise, judge, oracle, truth64
from gpuhelp import ctx, msdr, rel_rms  # noqa: F401
from test_gpu_f32_flavours import hilbert_pair, lowpass, sections
from test_gpu_out_i16 import to_q15

pytestmark = pytest.mark.gpu
F = msdr
LSB, USB, AM, CW = orclib.LSB, orclib.USB, orclib.AM, orclib.CW
COS4, SIN4 = np.array([1, 0, -1, 0], np.float32), np.array([0, 1, 0, -1], np.float32)
FS4 = (np.tile(SIN4, 32), np.tile(COS4, 32))
MFB = " (channel-batched block tiles)"
STREAM_LENS = [2 * 1024 + 32 + 5, 1024 + 77]


def cases():
    s = sections(oracle())
    S1, S2 = np.stack([s["lp"]]), np.stack([s["lp"], s["notch"]])
    S2N, S2R = np.stack([s["notch"], s["lp"]]), np.stack([s["lpr"], s["notch"]])
    env, ssb = (lowpass(100), lowpass(100, 2500.0)), hilbert_pair(100)
    ENV, SSB = F.FLAVOUR_ENV_UNITS | F.FLAVOUR_ENV_FOLD, F.FLAVOUR_SSB_UNITS | F.FLAVOUR_SSB_FOLD
    mfw = "chain_mfw_kernel<%d>"
    c = {}

    def add(name, kernel, flavour, env_scan, taps, bq, modes, lens=STREAM_LENS, seg=0, must_split=False, i16=False):
        c[name] = dict(name=name, kernel=kernel, flavour=flavour, env_scan=env_scan, taps=taps, bq=bq, modes=modes, lens=lens, seg=seg, must_split=must_split,
                       i16=i16, block=len(modes) > 3)

    add("am_lowpass_notch_rowlocal1", mfw % 2, ENV, 2, env, S2, [AM, CW, AM])               # the bench's cascade
    add("am_notch_lowpass_rowlocal2", mfw % 2, ENV, 3, env, S2N, [AM, CW, AM])
    add("am_two_resonant_scan_4x4", mfw % 2, ENV, 1, env, S2R, [AM, CW, AM])
    add("am_one_section", mfw % 1, ENV, 1, env, S1, [AM, CW, AM])
    add("lsb_one_section", mfw % 1, SSB, 0, ssb, S1, [LSB, USB, LSB])
    add("lsb_two_sections", mfw % 2, SSB, 0, ssb, S2, [LSB, USB, LSB])
    add("am_time_segments_2_n4133", mfw % 2, ENV, 2, env, S2, [AM, CW, AM], lens=[4096 + 37], seg=2)
    add("am_segmented_64k", mfw % 2, ENV, 2, env, S2, [AM, CW, AM], lens=[64 * 1024 + 37], seg=2, must_split=True)
    add("am_rowlocal1_int16_out", mfw % 2, ENV, 2, env, S2, [AM, CW, AM], i16=True)
    add("block_env_two_sections", "chain_mfb_kernel<2>" + MFB, F.FLAVOUR_BLOCK | ENV, 0, env, S2, [AM] * 33, lens=[128] * 5)
    add("block_lsb_two_sections", "chain_mfb_kernel<2>" + MFB, F.FLAVOUR_BLOCK | SSB, 0, ssb, S2, [LSB] * 33, lens=[128] * 5)
    return c


CASES = cases()
_REFS = {}


def inputs(e, n):
    """Row kinds in turn, as the census draws them: uniform full scale, |x| <= 40, sign-only +-32767; the int16-out case as tests/test_gpu_out_i16.py."""
    rng = np.random.default_rng([977, sorted(CASES).index(e["name"])])
    ch = len(e["modes"])
    if e["i16"]:
        return rng.integers(-20000, 20001, (ch, n)).astype(np.int16)
    x = np.empty((ch, n), np.int16)
    for c in range(ch):
        x[c] = (rng.integers(-32768, 32768, n) if c % 3 == 0 else rng.integers(-40, 41, n) if c % 3 == 1 else np.where(rng.integers(0, 2, n) > 0, 32767, -32767)).astype(np.int16)
    return x


def references(e, x, c):
    """(oracle, float64, oracle without cascade) of row c over the whole stream of the case's calls: computed once."""
    key = (e["name"], c)
    if key not in _REFS:
        a = (e["taps"][0], e["taps"][1], FS4[0], FS4[1])
        m = int(e["modes"][c])
        refs = (oracle().chain_f32(x[c], m, *a, e["bq"]), truth64(x[c], m, *a, e["bq"]), oracle().chain_f32(x[c], m, *a, None))
        for r in refs:
            r.setflags(write=False)
        _REFS[key] = refs
    return _REFS[key]


def judged_rows(e):
    ch = len(e["modes"])
    return list(range(ch)) if ch <= 8 else [0, 1, 2, 16, 31, 32]       # block tiles: the first and the last channel, and one inside, of every row kind


def windows(e, info):
    lens = e["lens"]
    if e["block"]:                      # a tick is too short to be judged alone while the FIR fills (the census's rule): the run and its last tick
        return [("all", slice(0, sum(lens))), ("last_tick", slice(sum(lens) - lens[-1], sum(lens)))]
    w, o = [], 0
    for k, n in enumerate(lens):
        w.append(("call%d" % k, slice(o, o + n)))
        o += n
    if info["time_segments"] > 1:
        n, t = lens[0], info["tile"]
        seg = -(-(-(-n // info["time_segments"])) // t) * t
        w += [("head", slice(0, 2048)), ("tail", slice(n - 1500, n))]
        w += [("boundary%d" % k, slice(k * seg - 512, k * seg + 512)) for k in range(1, info["time_segments"]) if k * seg + 64 <= n]
    return w


@pytest.mark.parametrize("name", sorted(CASES))
def test_kstacked_cascade_products(ctx, name):
    e = CASES[name]
    ch, lens = len(e["modes"]), e["lens"]
    x = inputs(e, sum(lens))
    chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, e["taps"][0], e["taps"][1], mixer=msdr.MIXER_FS4, modes=np.array(e["modes"], np.int32), biquad_coeffs=e["bq"],
                       time_segments=e["seg"], flags=msdr.CHAIN_OUT_I16 if e["i16"] else 0)
    dt = np.int16 if e["i16"] else np.float32
    got = np.empty((ch, sum(lens)), dt)
    o, first_info = 0, None
    for k, n in enumerate(lens):
        dx = ctx.to_device(np.ascontiguousarray(x[:, o:o + n]))
        fill = np.full((ch + 1, n), -12345 if e["i16"] else np.nan, dt)                 # every sample must be written; one guard row behind the last channel
        dy = ctx.to_device(fill)
        chain.process(dx, dy, n)
        y = dy.download()
        assert np.array_equal(y[ch], fill[ch], equal_nan=not e["i16"]), (name, k, "the guard row behind the last channel was written")
        if not e["i16"]:
            assert not np.isnan(y[:ch]).any(), (name, k, "NaN left in the output", np.argwhere(np.isnan(y[:ch]))[:4])
        got[:, o:o + n] = y[:ch]
        o += n
        info = chain.info()
        first_info = first_info or info
        print(name, "call", k, n, info)
        split = info["time_segments"] > 1
        want_flavour = e["flavour"] | (F.FLAVOUR_SEGMENTED if split else 0)
        assert (info["kernel"], info["flavour"], info["env_scan"]) == (e["kernel"], want_flavour, e["env_scan"]), (name, k, info)
        assert split == e["must_split"], (name, k, info["time_segments"])
    chain.close()
    for c in judged_rows(e):
        refs = references(e, x, c)
        if e["i16"]:                    # as tests/test_gpu_out_i16.py judges: never more than 1 LSB from the converted oracle, apart at all on under 1 % of the samples
            diff = np.abs(got[c].astype(np.int32) - to_q15(refs[0]).astype(np.int32))
            print("%s row %d max diff %d LSB, differing %.4f" % (name, c, int(diff.max()), float((diff != 0).mean())))
            assert diff.max() <= 1 and (diff != 0).mean() < 0.01, (name, c, int(diff.max()), float((diff != 0).mean()))
            continue
        case = dict(mode=int(e["modes"][c]), hi=e["taps"][0], hq=e["taps"][1], oi=FS4[0], oq=FS4[1], bq=e["bq"])
        noise = fp32_noise(e["bq"])
        for wname, w in windows(e, first_info):
            e_go, e_gpu, e_orc, bound = judge(got[c], x[c], case, refs=refs, window=w)
            b1 = 2 * e_orc + noise + 1e-6
            print("%s row %d %-10s e_go %.3e e_gpu %.3e e_orc %.3e bound %.3e ratio %.2f" % (name, c, wname, e_go, e_gpu, e_orc, b1, e_gpu / b1))
            assert e_go < 1e-5, (name, c, wname, "first clause", e_go)
            assert e_gpu <= min(bound, b1), (name, c, wname, "float64 clause: e_gpu %.3e e_orc %.3e fp32_noise %.2e bound %.3e" % (e_gpu, e_orc, noise, b1))
