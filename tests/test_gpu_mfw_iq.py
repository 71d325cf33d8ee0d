"""Q on accumulator 0's tap fragments in the wave-stream envelope kernels (mw_q_squares / burst_geom in
minimal-sdr_amd/csrc/msdr_chain_mfw.hiph, the table builder's check in msdr_iqshare.h).  Behind the exact Fs/4 mixer at an
even rotation, with one low-pass for I and Q, one tap-fragment read feeds both accumulators; Q arrives one sample late and is moved back
behind the burst, the sample in front of a tile travelling as a carry (the first tile of a unit computes its own).  Setup as in
tests/test_gpu_mfw_geom.py: MSDR_NO_BLOCK=1, 3 channels unless said, one full-scale row, the reference's two cascade sections.  Every case
runs as built and under MSDR_MFW_IQ=0 (every table keeps its own fragments for accumulator 1):

  * msdr_chain_get_iq_shared names the expected path for every call, and 0 under MSDR_MFW_IQ=0;
  * the default run meets the fp32 contract (tests/f32judge.py, both clauses, its tolerances);
  * its error against the oracle is at most twice the MSDR_MFW_IQ=0 run's (same products, some sums in another order: the margin
    tests/test_gpu_sparse24.py gives the merged steps);
  * on a shared call the two runs are NOT bit-identical (1/32 of the Q sums meet their chunks in another order), so the switch switches
    something; where no call shares (hQ != hI) they are.  The dense table (MSDR_MFW_SPARSE=0) is the one shared case where they must
    AGREE bit for bit: the sum that moves from (row a + 1, column 0) to (row a, column 31) meets the same window rows in the same order
    when every step is dense -- its empty first block and empty last block change places, and a zero product changes no sum; only the
    merged step, which takes a run's first and last chunk out of that order, makes the two differ.  On that one case nothing in the
    OUTPUT shows that the shared code ran: only msdr_chain_get_iq_shared says so (the host's word), and the run-time twin's shared path
    is shown to switch something by case 7 (MSDR_MFW_GEOM=0 with merged steps), which runs the same kernel;
  * the carried FIR history is identical;
  * with MSDR_MFW_GEOM=0 the run-time twin shares as well and agrees with the constant-geometry kernel bit for bit."""
import numpy as np
import pytest

import orclib
from f32judge import judge, oracle, truth64
from gpuhelp import ctx, msdr  # noqa: F401
from test_gpu_f32_flavours import lowpass
from test_gpu_mfw_geom import FS4, TOL, _s2, df1_64, synth

pytestmark = pytest.mark.gpu
AM = orclib.AM


def cases():
    """name -> channels, taps, calls, time_segments, environment, expected iq_shared and geometry per call of the default run, `then`:
    the live update before call k ("equal": set_taps to another equal pair, "unequal": to hI != hQ), hq: "same" or "other"."""
    c = {}

    def add(name, ch, ntaps, lens, iq, geom, seg=0, env=None, then=None, hq="same"):
        c[name] = dict(name=name, ch=ch, ntaps=ntaps, lens=lens, iq=iq, geom=geom, seg=seg, env=env or {}, then=then or {}, hq=hq)

    # hot last tile; the second call takes real history into its first tile's carry
    add("1_hot_last_tile_then_second_call", 3, 256, [3072, 2048], [1, 1], [1, 1])
    # two workgroups, cold tail, misaligned rows
    add("2_two_workgroups_cold_tail", 19, 256, [5420], [1], [1])
    # all cold; the second call starts at an odd rotation, whose tables swap the arrays: refused there
    add("3_all_cold_then_odd_rotation", 3, 256, [3075, 1100], [1, 0], [1, 0])
    add("4_time_segments_2", 3, 256, [1 << 16], [1], [1], seg=2)
    add("5_512_taps", 3, 512, [4096 + 300, 1024], [1, 1], [2, 2])
    add("6_dense_table", 3, 256, [4096 + 300, 1024], [1, 1], [0, 0], env={"MSDR_MFW_SPARSE": "0"})
    add("7_run_time_twin", 3, 256, [3072, 2048 + 300], [1, 1], [0, 0], env={"MSDR_MFW_GEOM": "0"})
    add("8_hq_differs_refused", 3, 256, [3072, 1024 + 300], [0, 0], [0, 0], hq="other")
    add("9_live_set_taps_to_an_equal_pair", 3, 256, [3072, 2048 + 300], [1, 1], [1, 1], then={1: "equal"})
    add("10_live_set_taps_to_an_unequal_pair", 3, 256, [3072, 2048 + 300], [1, 0], [1, 0], then={1: "unequal"})
    add("11_live_set_taps_from_unequal_to_equal", 3, 256, [3072, 2048 + 300], [0, 1], [0, 1], then={1: "equal"}, hq="other")
    return c


CASES = cases()
ENV = ("MSDR_MFW_GEOM", "MSDR_MFW_SPARSE", "MSDR_MFW_IQ")


def run(ctx, monkeypatch, e, x, pairs, bq, iq_on, extra_env=None):
    """pairs: the (hI, hQ) of every call.  -> outputs, info, geometry, iq_shared, carried FIR history, per call."""
    monkeypatch.setenv("MSDR_NO_BLOCK", "1")
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(e["env"], **(extra_env or {})).items():
        monkeypatch.setenv(k, v)
    if not iq_on:
        monkeypatch.setenv("MSDR_MFW_IQ", "0")
    ch = e["ch"]
    chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, pairs[0][0], pairs[0][1], mixer=msdr.MIXER_FS4, modes=np.full(ch, AM, np.int32), biquad_coeffs=bq,
                       time_segments=e["seg"])
    assert chain.iq_shared() == 0                                             # before the first call
    outs, infos, geoms, iqs, hists = [], [], [], [], []
    o = 0
    for k, n in enumerate(e["lens"]):
        if k in e["then"]:
            chain.set_taps(0, pairs[k][0], pairs[k][1])
        dx = ctx.to_device(np.ascontiguousarray(x[:, o:o + n]))
        dy = ctx.to_device(np.full((ch + 1, n), np.nan, np.float32))          # every sample must be written; one guard row behind the last channel
        chain.process(dx, dy, n)
        y = dy.download()
        assert np.isnan(y[ch]).all(), (e["name"], k, "the guard row behind the last channel was written")
        assert not np.isnan(y[:ch]).any(), (e["name"], k, "NaN left in the output")
        outs.append(y[:ch])
        infos.append(chain.info())
        geoms.append(chain.geometry())
        iqs.append(chain.iq_shared())
        hists.append(np.stack([chain.fir_history(c) for c in range(min(ch, 3))]))
        o += n
    chain.close()
    return outs, infos, geoms, iqs, hists


def pairs_of(e):
    taps, other, taps2 = lowpass(e["ntaps"]), lowpass(e["ntaps"], 2500.0), lowpass(e["ntaps"], 2200.0)
    first = (taps, taps if e["hq"] == "same" else other)
    out = [first]
    for k in range(1, len(e["lens"])):
        what = e["then"].get(k)
        out.append((taps2, taps2) if what == "equal" else (taps2, other) if what == "unequal" else out[-1])
    return out


def reference_rows(x_row, pairs, lens, bq):
    """(oracle, float64, oracle without the cascade) of one row whose taps change at the call boundaries: FIR and demodulator of each part
    on the whole row (the history is the samples), spliced; the cascade runs over the splice with its state carried across."""
    orc = oracle()
    starts = np.concatenate([[0], np.cumsum(lens)])
    pre64 = np.concatenate([truth64(x_row, AM, p[0], p[1], FS4[0], FS4[1], None)[starts[k]:starts[k + 1]] for k, p in enumerate(pairs)])
    pre = np.concatenate([orc.chain_f32(x_row, AM, p[0], p[1], FS4[0], FS4[1], None)[starts[k]:starts[k + 1]] for k, p in enumerate(pairs)])
    st = {}
    want = np.concatenate([orc.chain_f32(x_row[starts[k]:starts[k + 1]], AM, p[0], p[1], FS4[0], FS4[1], bq, state=st) for k, p in enumerate(pairs)])
    return want, df1_64(pre64, [(0, bq)]), pre


def check(name, e, x, pairs, bq, got, ref, rows):
    """The contract of the default run and its error against the MSDR_MFW_IQ=0 run's, per row and call."""
    lens = e["lens"]
    starts = np.concatenate([[0], np.cumsum(lens)])
    changing = any(p is not pairs[0] for p in pairs)
    for c in rows:
        if changing:
            refs = reference_rows(x[c], pairs, lens, bq)
        else:
            a = (pairs[0][0], pairs[0][1], FS4[0], FS4[1])
            refs = (oracle().chain_f32(x[c], AM, *a, bq), truth64(x[c], AM, *a, bq), oracle().chain_f32(x[c], AM, *a, None))
        case = dict(mode=AM, hi=pairs[-1][0], hq=pairs[-1][1], oi=FS4[0], oq=FS4[1], bq=bq)
        row, row0 = np.concatenate([g[c] for g in got]), np.concatenate([g[c] for g in ref])
        for k in range(len(lens)):
            w = slice(int(starts[k]), int(starts[k + 1]))
            e_go, e_gpu, e_orc, bound = judge(row, x[c], case, refs=refs, window=w)
            e_go0 = judge(row0, x[c], case, refs=refs, window=w)[0]
            print("%s row %d call %d: gpu-oracle %.3e (MSDR_MFW_IQ=0: %.3e) gpu-f64 %.3e oracle-f64 %.3e bound %.3e" % (name, c, k, e_go, e_go0, e_gpu, e_orc, bound))
            assert e_go < TOL, (name, c, k, "first clause", e_go)
            assert e_gpu <= bound, (name, c, k, "second clause", e_gpu, bound)
            assert e_go <= 2 * e_go0, (name, c, k, "error against the oracle more than twice the unshared run's", e_go, e_go0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_q_on_accumulator_0s_fragments_against_its_own_fragments_and_the_oracle(ctx, monkeypatch, name):
    e = CASES[name]
    ch, lens = e["ch"], e["lens"]
    x = synth(np.random.default_rng([11, sorted(CASES).index(name)]), ch, sum(lens))
    pairs, bq = pairs_of(e), _s2()
    got, info, geom, iq, hist = run(ctx, monkeypatch, e, x, pairs, bq, True)
    ref, info0, geom0, iq0, hist0 = run(ctx, monkeypatch, e, x, pairs, bq, False)
    for k in range(len(lens)):
        same = np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32))
        print(name, "call", k, "iq_shared", iq[k], "geometry", geom[k], "with MSDR_MFW_IQ=0:", iq0[k], geom0[k], "bit-identical" if same else "differ", info[k]["kernel"])
        assert info[k]["kernel"].startswith("chain_mfw_kernel<2>") and info[k] == info0[k], (name, k, info[k], info0[k])
        assert iq[k] == e["iq"][k] and geom[k] == e["geom"][k], (name, k, "iq_shared", iq[k], "geometry", geom[k], "expected", e["iq"][k], e["geom"][k])
        assert iq0[k] == 0 and geom0[k] == 0, (name, k, "MSDR_MFW_IQ=0 ran", iq0[k], geom0[k])      # (the instantiated kernels exist shared only)
        if iq[k] and e["env"].get("MSDR_MFW_SPARSE") == "0":
            assert same, (name, k, "every step dense: the shared run must agree with the unshared one bit for bit")
        elif iq[k]:
            assert not same, (name, k, "the shared and the unshared run agree bit for bit: nothing was switched")
        elif not any(e["iq"][:k]):
            assert same, (name, k, "no call shared so far, yet the two runs differ")
        assert np.array_equal(hist[k], hist0[k]), (name, k, "carried FIR history differs")
    if e["env"].get("MSDR_MFW_GEOM") == "0":
        # the run-time twin against the constant-geometry kernel, both shared: bit for bit
        geo, _, geom1, iq1, hist1 = run(ctx, monkeypatch, e, x, pairs, bq, True, extra_env={"MSDR_MFW_GEOM": "1"})
        for k in range(len(lens)):
            assert geom1[k] == 1 and iq1[k] == 1, (name, k, geom1[k], iq1[k])
            assert np.array_equal(got[k].view(np.uint32), geo[k].view(np.uint32)), (name, k, "run-time twin and constant geometry differ")
            assert np.array_equal(hist[k], hist1[k]), (name, k)
    check(name, e, x, pairs, bq, got, ref, range(ch) if ch <= 3 else (0, 1, 2, 15, 16, 18))


def test_one_hot_rows_meet_every_tap_at_its_own_sample(ctx, monkeypatch):
    """Single impulses, 700 samples apart (moved by up to 31 to reach an offset), at even and at odd positions (the I and the Q stream) and at many offsets inside the
    32-sample rows -- b = 0 and b = 31 among them, and a tile's first and last sample --, through an ASYMMETRIC equal pair: every output
    sample is one tap's magnitude run through the cascade, so a Q that is one sample early or late, or a carry lost at a row or tile
    edge, shows as the wrong tap.  No flavour without a cascade takes the shared path (its halo has no spare chunk in front: the check
    refuses runs from chunk 0), so the reference's two sections run and the oracle is the reference.  Pointwise bound: 1e-4 of the row's
    peak -- the fp32 chain is within about 1e-6 of the oracle there, a neighbouring tap is off by the filter's slope, 1e-3 and more of the
    peak around the main lobe."""
    e = dict(name="one_hot", ch=3, lens=[14336], seg=0, env={}, then={})
    n = e["lens"][0]
    residues = [0, 31, 1, 30, 16, 15, 17, 2, 29, 14, 3, 28]
    pos = []
    for k, r in enumerate(residues):
        p = 350 + 700 * k
        pos.append(p + (r - p) % 32)
    pos += [10240, 11263, 12287, 13312]                                       # a tile's first sample, two tiles' last samples, a first sample again
    assert all(b - a >= 700 - 31 for a, b in zip(pos, pos[1:])) and {p & 1 for p in pos} == {0, 1} and {0, 31} <= {p % 32 for p in pos}
    assert {0, 1023} <= {p % 1024 for p in pos}
    x = synth(np.random.default_rng(5), 3, n)
    x[0] = 0
    x[0, pos] = np.where(np.arange(len(pos)) % 3 == 0, -20000, 20000).astype(np.int16)
    taps = (lowpass(256) * (1 + 0.5 * np.arange(256) / 256)).astype(np.float32)
    pairs, bq = [(taps, taps)], _s2()
    got, _, geom, iq, _ = run(ctx, monkeypatch, e, x, pairs, bq, True)
    ref, _, _, iq0, _ = run(ctx, monkeypatch, e, x, pairs, bq, False)
    assert iq == [1] and geom == [1] and iq0 == [0], (iq, geom, iq0)
    want = oracle().chain_f32(x[0], AM, taps, taps, FS4[0], FS4[1], bq)
    peak = float(np.abs(want).max())
    err, err0 = np.abs(got[0][0] - want), np.abs(ref[0][0] - want)
    print("one-hot row: peak %.3e, worst |gpu - oracle| %.3e at sample %d (MSDR_MFW_IQ=0: %.3e)" % (peak, err.max(), int(err.argmax()), err0.max()))
    assert err.max() <= 1e-4 * peak, ("a tap at the wrong sample", int(err.argmax()), float(err.max()), peak)
    check("one_hot", e, x, pairs, bq, got, ref, range(3))
