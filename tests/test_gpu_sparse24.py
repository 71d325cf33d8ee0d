"""The wave-stream chain's merged k-step: the first and the last 16-sample step of a FIR run issued as ONE 2:4-sparse matrix product
(v_smfmac_f32_32x32x32_f16; minimal-sdr_amd/csrc/msdr_sparse24.h).  Every case runs twice on the same input -- as built, and
created under MSDR_MFW_SPARSE=0 (every run dense) -- with MSDR_NO_BLOCK=1 so that the wave-stream kernel takes both calls: 5 channels, the Fs/4
mixer, a call of 4096 + 300 samples continued by one of 1024 + 77 (hot tiles, cold tails, an unaligned second call, the state and history
hand-off).  Rows: one of full-scale samples (+-32767 and -32768), one of |x| < 32, three of two tones + noise (bench.py's synth_if).

Judged per channel and call against the fp32 oracle's chain_f32: relative RMS <= 1e-5 (the project's tolerance) on both paths, and the
sparse path's error at most twice the dense path's (the same products in fp32; two of a run's steps change their place in the sum).
info()["mfma_ksteps"] counts a merged step once: it drops by the number of merged runs where the tables must merge (every Toeplitz envelope
table: two runs), and tells which path ran where the host may refuse (the SSB table with two folded sections).

The last test is the layout check of tools/probes/smfmac_probe through the library, reduced: one-hot inputs, whose outputs are the taps
themselves, at window positions that meet the merged step's first and last block in every lane half and K group."""
import numpy as np
import pytest

import orclib
from f32judge import oracle
from gpuhelp import ctx, msdr, rel_rms  # noqa: F401
from test_gpu_f32_flavours import hilbert_pair, lowpass, sections

pytestmark = pytest.mark.gpu
LSB, AM = orclib.LSB, orclib.AM
COS4, SIN4 = np.array([1, 0, -1, 0], np.float32), np.array([0, 1, 0, -1], np.float32)
FS4 = (np.tile(SIN4, 32), np.tile(COS4, 32))
CH = 5
LENS = [4096 + 300, 1024 + 77]
TOL = 1e-5


def cases():
    s = sections(oracle())
    S2 = np.stack([s["lp"], s["notch"]])                    # the reference's two sections (the bench's cascade)
    c = {}

    def add(name, mode, taps, bq, merged, seg=0):
        c[name] = dict(name=name, mode=mode, taps=taps, bq=bq, merged=merged, seg=seg)

    add("am_256_two_sections_rowlocal", AM, (lowpass(256), lowpass(256)), S2, 2)
    # (256 taps with at most one section and the SAME low-pass for I and Q go to chain_amtr_kernel: these take two bandwidths)
    add("am_256_no_sections", AM, (lowpass(256), lowpass(256, 2500.0)), None, 2)
    add("am_64", AM, (lowpass(64), lowpass(64)), None, 2)            # three steps a run: one merged + one dense
    add("am_24", AM, (lowpass(24), lowpass(24)), None, 2)            # two steps a run: the merged step alone
    add("am_512", AM, (lowpass(512), lowpass(512)), None, 2)
    add("lsb_hilbert_100_two_sections", LSB, hilbert_pair(100), S2, None)      # folded numerator and cascade in the columns: the host may refuse
    add("am_256_time_segments_2", AM, (lowpass(256), lowpass(256, 2500.0)), None, 2, seg=2)
    return c


CASES = cases()


def synth_if(rng, n):
    """bench.py's synth_if on the host: two tones (6.7 kHz, 5.4 kHz at -6 dB) + uniform noise +-500."""
    t = np.arange(n, dtype=np.float64)
    v = 6000.0 * np.cos(t * (2 * np.pi * 6700.0 / 24000.0)) + 3000.0 * np.cos(t * (2 * np.pi * 5400.0 / 24000.0) + 0.3)
    return np.round(v + rng.integers(-500, 501, n)).astype(np.int16)


def inputs(seed, n):
    rng = np.random.default_rng([2024, seed])
    x = np.empty((CH, n), np.int16)
    x[0] = rng.choice(np.array([32767, -32767, -32768], np.int16), n)
    x[1] = rng.integers(-31, 32, n).astype(np.int16)
    for c in range(2, CH):
        x[c] = synth_if(rng, n)
    return x


def run_chain(ctx, monkeypatch, e, x, sparse, lens=LENS):
    monkeypatch.setenv("MSDR_NO_BLOCK", "1")
    if sparse:
        monkeypatch.delenv("MSDR_MFW_SPARSE", raising=False)
    else:
        monkeypatch.setenv("MSDR_MFW_SPARSE", "0")
    chain = msdr.Chain(ctx, msdr.ARITH_F32, CH, e["taps"][0], e["taps"][1], mixer=msdr.MIXER_FS4, modes=np.full(CH, e["mode"], np.int32),
                       biquad_coeffs=e["bq"], time_segments=e["seg"])
    got = np.empty((CH, sum(lens)), np.float32)
    o, infos = 0, []
    for n in lens:
        dx = ctx.to_device(np.ascontiguousarray(x[:, o:o + n]))
        fill = np.full((CH + 1, n), np.nan, np.float32)               # every sample must be written; one guard row behind the last channel
        dy = ctx.to_device(fill)
        chain.process(dx, dy, n)
        y = dy.download()
        assert np.isnan(y[CH]).all(), (e["name"], "the guard row behind the last channel was written")
        assert not np.isnan(y[:CH]).any(), (e["name"], "NaN left in the output", np.argwhere(np.isnan(y[:CH]))[:4])
        got[:, o:o + n] = y[:CH]
        o += n
        infos.append(chain.info())
    chain.close()
    return got, infos


@pytest.mark.parametrize("name", sorted(CASES))
def test_merged_step_against_the_oracle_and_the_dense_path(ctx, monkeypatch, name):
    e = CASES[name]
    x = inputs(sorted(CASES).index(name), sum(LENS))
    refs = [oracle().chain_f32(x[c], e["mode"], e["taps"][0], e["taps"][1], FS4[0], FS4[1], e["bq"]) for c in range(CH)]
    got_s, info_s = run_chain(ctx, monkeypatch, e, x, True)
    got_d, info_d = run_chain(ctx, monkeypatch, e, x, False)
    for k in range(len(LENS)):
        print(name, "call", k, "sparse", info_s[k], "dense", info_d[k])
        assert info_s[k]["kernel"].startswith("chain_mfw_kernel") and info_d[k]["kernel"] == info_s[k]["kernel"], (name, k, info_s[k], info_d[k])
        drop = info_d[k]["mfma_ksteps"] - info_s[k]["mfma_ksteps"]
        if e["merged"] is None:
            assert drop in (0, 1, 2), (name, k, drop)
            print(name, "call", k, "the host %s: mfma_ksteps %d -> %d" % ("merged %d runs" % drop if drop else "refused", info_d[k]["mfma_ksteps"], info_s[k]["mfma_ksteps"]))
        else:
            assert drop == e["merged"], (name, k, "merged runs", drop, info_d[k]["mfma_ksteps"], info_s[k]["mfma_ksteps"])
    o = 0
    for k, n in enumerate(LENS):
        for c in range(CH):
            w = slice(o, o + n)
            es, ed = rel_rms(got_s[c, w], refs[c][w]), rel_rms(got_d[c, w], refs[c][w])
            print("%s row %d call %d: sparse %.3e dense %.3e ratio %.2f" % (name, c, k, es, ed, es / max(ed, 1e-300)))
            assert ed <= TOL, (name, c, k, "dense path", ed)
            assert es <= TOL, (name, c, k, "sparse path", es)
            assert es <= 2.0 * ed, (name, c, k, "sparse path's error above twice the dense path's", es, ed)
        o += n


def test_one_hot_inputs_give_the_taps_through_the_merged_step(ctx, monkeypatch):
    """An envelope channel fed a single sample answers with |tap| x sample: impulses 700 samples apart (further than the 256 taps), at even and
    odd positions and at many offsets inside the 32-sample rows, so that the entries of the merged step's two blocks each carry a tap to an
    output of their own.  Asymmetric taps, different for I and Q (a symmetric filter would hide a reversed K order)."""
    n = 4096 + 300
    h = (lowpass(256) * (1.0 + 0.5 * np.arange(256) / 256.0)).astype(np.float32)
    hq = (lowpass(256, 2500.0) * (1.5 - 0.5 * np.arange(256) / 256.0)).astype(np.float32)
    e = dict(name="one_hot", mode=AM, taps=(h, hq), bq=None, seg=0)
    x = np.zeros((CH, n), np.int16)
    for c in range(CH):
        for k, p in enumerate(range(40 + 7 * c, n - 300, 700 + c)):
            x[c, p + (k % 2)] = 16384 if (k + c) % 2 else -12000
    got, infos = run_chain(ctx, monkeypatch, e, x, True, lens=[n])
    dense, infod = run_chain(ctx, monkeypatch, e, x, False, lens=[n])
    assert infod[0]["mfma_ksteps"] - infos[0]["mfma_ksteps"] == 2, (infos, infod)
    for c in range(CH):
        ref = oracle().chain_f32(x[c], AM, h, hq, FS4[0], FS4[1], None)
        err, peak = np.abs(got[c].astype(np.float64) - ref), np.abs(ref).max()
        print("one-hot row %d: rel rms %.3e (dense %.3e), max abs error %.3e of peak %.3e" % (c, rel_rms(got[c], ref), rel_rms(dense[c], ref), err.max(), peak))
        assert rel_rms(got[c], ref) <= TOL, (c, rel_rms(got[c], ref))
        # a tap in the wrong place is an error of the size of a tap: every output within 1e-4 of the largest response
        assert err.max() <= 1e-4 * peak, (c, int(err.argmax()), err.max(), peak)
