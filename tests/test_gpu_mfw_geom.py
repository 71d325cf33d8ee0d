"""The wave-stream envelope kernel with the run geometry of its tap tables as compile-time constants (chain_mfw_geom_kernel, MwGeom in
minimal-sdr_amd/csrc/msdr_chain_mfw.hiph).  Every case runs twice in the same library on the same input -- as built, and
created under MSDR_MFW_GEOM=0 (the kernels that read the geometry from the table headers) -- with MSDR_NO_BLOCK=1 so that the wave-stream
kernel takes the short calls.  The two runs must agree bit for bit, call by call (a continuing call consumes the state and the history the
call before handed over; the carried FIR history is compared as well), the default run must meet the fp32 contract against the oracle
(tests/f32judge.py), and msdr_chain_get_geometry must name the expected path for every call: a test cannot pass by running the other kernel.

Configuration unless a case says otherwise: envelope (AM) channels behind the exact Fs/4 mixer, one 256-tap low-pass for I and Q, the
reference's two cascade sections (low-pass Q 0.54 + notch: section 0 row-local) -- c3's kernel and geometry 1; 512 taps: geometry 2."""
import numpy as np
import pytest

import orclib
from f32judge import judge, oracle, truth64
from gpuhelp import ctx, msdr  # noqa: F401
from test_gpu_f32_flavours import lowpass, sections

pytestmark = pytest.mark.gpu
AM = orclib.AM
COS4, SIN4 = np.array([1, 0, -1, 0], np.float32), np.array([0, 1, 0, -1], np.float32)
FS4 = (np.tile(SIN4, 32), np.tile(COS4, 32))
TOL = 1e-5


def _s2():
    s = sections(oracle())
    return np.stack([s["lp"], s["notch"]])


def _s2_resonant():
    s = sections(oracle())
    return np.stack([s["lpr"], s["notch"]])


def cases():
    """name -> channels, taps, the calls' lengths, time_segments, environment, the expected geometry per call (default run), and
    `then`: what happens before call k (a live update)."""
    c = {}

    def add(name, ch, ntaps, lens, geom, seg=0, env=None, then=None, scan=None):
        c[name] = dict(name=name, ch=ch, ntaps=ntaps, lens=lens, geom=geom, seg=seg, env=env or {}, then=then or {}, scan=scan)

    # two workgroups (16 waves each at 256 taps), the second with idle units; five full tiles and a cold tail; odd channels' rows misaligned
    add("1_two_workgroups_cold_tail", 19, 256, [5420], [1])
    # last tile hot, state capture in a hot tile; the second call takes the state and the history over
    add("2_4_aligned_last_tile_hot_then_second_call", 3, 256, [3072, 2048], [1, 1])
    # odd n: the rows of channel >= 1 are misaligned, all cold tiles; the call behind it starts at an odd oscillator rotation, whose tables
    # swap the window arrays: no instantiation, the run-time kernel
    add("3_odd_n_all_cold_then_odd_rotation", 3, 256, [3075, 1100], [1, 0])
    add("5_time_segments_2", 3, 256, [1 << 15], [1], seg=2)
    # (at 2^15 samples the host keeps one segment: a segment is at least 32 warm-up tiles long.  2^16 is the smallest call it splits)
    add("5_time_segments_2_split", 3, 256, [1 << 16], [1], seg=2, scan="segmented")
    add("6_512_taps", 3, 512, [4096 + 300, 1024], [2, 2])
    add("7_230_taps_no_instantiation", 3, 230, [4096 + 300, 1024], [0, 0])
    add("8_dense_table", 3, 256, [4096 + 300, 1024], [0, 0], env={"MSDR_MFW_SPARSE": "0"})
    add("9_live_set_taps_same_length", 3, 256, [3072, 2048 + 300], [1, 1], then={1: "taps"})
    add("10_live_cascade_to_two_resonant_sections", 3, 256, [3072, 2048 + 300], [1, 0], then={1: "cascade"}, scan=[2, 1])
    return c


CASES = cases()


def synth(rng, ch, n):
    t = np.arange(n, dtype=np.float64)
    x = np.empty((ch, n), np.int16)
    for c in range(ch):
        v = 6000.0 * np.cos(t * (2 * np.pi * (6700.0 + 13.0 * c) / 24000.0)) + 3000.0 * np.cos(t * (2 * np.pi * 5400.0 / 24000.0) + 0.3 * c)
        x[c] = np.round(v + rng.integers(-500, 501, n)).astype(np.int16)
    if ch > 2:
        x[1] = rng.choice(np.array([32767, -32767, -32768], np.int16), n)       # a full-scale row
    return x


def df1_64(d, plan):
    """The cascade in float64, direct form 1, the state (past inputs and outputs of every section) carried over a change of
    coefficients: plan = [(first sample, coefficient rows b0 b1 b2 a1 a2 with a's as the library takes them), ...]."""
    y = np.asarray(d, np.float64).copy()
    S = len(plan[0][1])
    for s in range(S):
        x1 = x2 = y1 = y2 = 0.0
        out = np.empty_like(y)
        for k, (lo, bq) in enumerate(plan):
            hi = plan[k + 1][0] if k + 1 < len(plan) else y.size
            b0, b1, b2, a1, a2 = (float(v) for v in np.asarray(bq, np.float64)[s])
            for n in range(lo, hi):
                v = y[n]
                w = b0 * v + b1 * x1 + b2 * x2 + a1 * y1 + a2 * y2
                x2, x1, y2, y1 = x1, v, y1, w
                out[n] = w
        y = out
    return y


def run(ctx, monkeypatch, e, x, taps, taps2, bq, bq2, geom_on):
    monkeypatch.setenv("MSDR_NO_BLOCK", "1")
    for k in ("MSDR_MFW_GEOM", "MSDR_MFW_SPARSE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in e["env"].items():
        monkeypatch.setenv(k, v)
    if not geom_on:
        monkeypatch.setenv("MSDR_MFW_GEOM", "0")
    ch = e["ch"]
    chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, taps, taps, mixer=msdr.MIXER_FS4, modes=np.full(ch, AM, np.int32), biquad_coeffs=bq,
                       time_segments=e["seg"])
    outs, infos, geoms, hists = [], [], [], []
    o = 0
    for k, n in enumerate(e["lens"]):
        if e["then"].get(k) == "taps":
            chain.set_taps(0, taps2, taps2)
        if e["then"].get(k) == "cascade":
            chain.set_biquad_coeffs(bq2)
        dx = ctx.to_device(np.ascontiguousarray(x[:, o:o + n]))
        dy = ctx.to_device(np.full((ch + 1, n), np.nan, np.float32))          # every sample must be written; one guard row behind the last channel
        chain.process(dx, dy, n)
        y = dy.download()
        assert np.isnan(y[ch]).all(), (e["name"], k, "the guard row behind the last channel was written")
        assert not np.isnan(y[:ch]).any(), (e["name"], k, "NaN left in the output")
        outs.append(y[:ch])
        infos.append(chain.info())
        geoms.append(chain.geometry())
        hists.append(np.stack([chain.fir_history(c) for c in range(min(ch, 3))]))
        o += n
    chain.close()
    return outs, infos, geoms, hists


@pytest.mark.parametrize("name", sorted(CASES))
def test_constant_geometry_against_the_run_time_path_and_the_oracle(ctx, monkeypatch, name):
    e = CASES[name]
    ch, lens, total = e["ch"], e["lens"], sum(e["lens"])
    x = synth(np.random.default_rng([7, sorted(CASES).index(name)]), ch, total)
    taps, taps2 = lowpass(e["ntaps"]), lowpass(e["ntaps"], 2200.0)
    bq, bq2 = _s2(), _s2_resonant()
    got, info, geom, hist = run(ctx, monkeypatch, e, x, taps, taps2, bq, bq2, True)
    ref, info0, geom0, hist0 = run(ctx, monkeypatch, e, x, taps, taps2, bq, bq2, False)
    for k in range(len(lens)):
        print(name, "call", k, "geometry", geom[k], "with MSDR_MFW_GEOM=0", geom0[k], info[k])
        assert info[k]["kernel"].startswith("chain_mfw_kernel<2>") and info[k] == info0[k], (name, k, info[k], info0[k])
        assert geom[k] == e["geom"][k], (name, k, "geometry", geom[k], "expected", e["geom"][k])
        assert geom0[k] == 0, (name, k, "MSDR_MFW_GEOM=0 ran geometry", geom0[k])
        if isinstance(e["scan"], list):
            assert info[k]["env_scan"] == e["scan"][k], (name, k, info[k])
        elif e["scan"] == "segmented":
            assert info[k]["time_segments"] > 1 and info[k]["warmup"] > 0, (name, k, info[k])
        else:
            assert info[k]["env_scan"] == 2, (name, k, info[k])               # section 0 row-local: c3's kernel
        assert np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), (name, k, "outputs differ between the two paths",
                                                                                 int((got[k].view(np.uint32) != ref[k].view(np.uint32)).sum()))
        assert np.array_equal(hist[k], hist0[k]), (name, k, "carried FIR history differs")
    # ---- the fp32 contract, per channel and call, on the rows as they continue over the calls ----
    orc = oracle()
    starts = np.concatenate([[0], np.cumsum(lens)])
    rows = range(ch) if ch <= 3 else (0, 1, 2, 15, 16, 18)                   # (19 channels: both workgroups, aligned and misaligned rows)
    for c in rows:
        if e["then"]:
            # a live update before call 1: FIR and demodulator of each part on the whole row (the history is the samples), spliced at the
            # call boundary; the cascade then runs over the splice with its state carried across the change
            cut = int(starts[1])
            tp = [taps, taps2 if "taps" in e["then"].values() else taps]
            plan = [(0, bq), (cut, bq2 if "cascade" in e["then"].values() else bq)]
            pre64 = np.concatenate([truth64(x[c], AM, tp[0], tp[0], FS4[0], FS4[1], None)[:cut], truth64(x[c], AM, tp[1], tp[1], FS4[0], FS4[1], None)[cut:]])
            pre = np.concatenate([orc.chain_f32(x[c], AM, tp[0], tp[0], FS4[0], FS4[1], None)[:cut], orc.chain_f32(x[c], AM, tp[1], tp[1], FS4[0], FS4[1], None)[cut:]])
            st = {}
            want = np.concatenate([orc.chain_f32(x[c, :cut], AM, tp[0], tp[0], FS4[0], FS4[1], plan[0][1], state=st),
                                   orc.chain_f32(x[c, cut:], AM, tp[1], tp[1], FS4[0], FS4[1], plan[1][1], state=st)])
            refs = (want, df1_64(pre64, plan), pre)
            case = dict(mode=AM, hi=taps, hq=taps, oi=FS4[0], oq=FS4[1], bq=plan[1][1])
        else:
            case = dict(mode=AM, hi=taps, hq=taps, oi=FS4[0], oq=FS4[1], bq=bq)
            refs = (orc.chain_f32(x[c], AM, taps, taps, FS4[0], FS4[1], bq), truth64(x[c], AM, taps, taps, FS4[0], FS4[1], bq),
                    orc.chain_f32(x[c], AM, taps, taps, FS4[0], FS4[1], None))
        row = np.concatenate([g[c] for g in got])
        for k in range(len(lens)):
            e_go, e_gpu, e_orc, bound = judge(row, x[c], case, refs=refs, window=slice(int(starts[k]), int(starts[k + 1])))
            print("%s row %d call %d: gpu-oracle %.3e gpu-f64 %.3e oracle-f64 %.3e bound %.3e" % (name, c, k, e_go, e_gpu, e_orc, bound))
            assert e_go < TOL, (name, c, k, "first clause", e_go)
            assert e_gpu <= bound, (name, c, k, "second clause", e_gpu, bound)
