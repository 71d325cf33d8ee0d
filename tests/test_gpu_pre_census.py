"""The census of the two-stage decimating chain kernels, Q15 half: one case per Q15 entry of tests/pre_census_cases.py -- every launch geometry
pre_geometry can hand chain_q15pcn2_kernel (69 keys, D1 rotating so that every stage-1 read width runs at every lane count), every (CPW, AL)
instantiation of the _full twin with meter, pairs and gain switched on in turn, the prefilter lengths around a step of 8, the limits of both
setters, stage 1's saturation and wrap behind every D1 and one call in two time segments per tile.

Every entry runs the recipe of the other censuses (tests/test_gpu_decim_census.py::run_entry, with this table's stream, calls and reading of
chain.info()): CPW * waves + 1 channels of mixed modes, three calls over one stream from the clear state -- the entry's length, 2 outputs, the
entry's length again --, audio, pairs and meter of every call in buffers filled with a sentinel between guard stretches.

Everything is int16 / uint64 and exact (np.array_equal): tests/prefilter_model.py::model_q15 over the whole stream gives audio and pairs, the
meter is tests/test_gpu_meter_per_channel.py::sums over the pairs of each call; a gained entry is held to tests/agc_model.py -- the stage-2
accumulators over the oracle's stage-1 intermediates, the multiplier, and the receivers' records behind every call.  WHICH code ran is read
from chain.info() after the first and the last call: the family's name, block == 64 waves, tile == opl * 64 / CPW and lds_bytes == the rule's
figure.  The Q15 twins have no flavour word: that the tap's, the meter's and the records' buffers hold the model's values, and nothing
around them changed, is the evidence."""
import numpy as np
import pytest

import agc_model as agc
import pre_census_cases as cases
import prefilter_model as pm
from gpuhelp import ctx, msdr  # noqa: F401
from test_gpu_decim_census import raw, refusal, run_entry
from test_gpu_decim_per_channel import nco_chain
from test_gpu_meter_per_channel import sums
from test_gpu_nco_per_channel import Bank

pytestmark = pytest.mark.gpu
I16 = np.int16
_REFS = {}


def ran(info, e):
    """which code ran, from chain.info() alone"""
    assert info["kernel"].startswith(cases.stem(e["f32"])), info
    assert info["block"] == 64 * e["nw"] and info["tile"] == e["opl"] * 64 // e["cpw"] == e["tile"], (info, e)
    assert info["lds_bytes"] == e["lds"], (info, e)
    if e["part"] == "F":
        assert info["time_segments"] == e["nseg"] >= 2, (info, e)


def osc(e):
    d = cases.data(e)
    return Bank(d["steps"], d["phases"]).advance(d["n"])


def refs_q15(orc, e):
    """per channel dict(audio, fi, fq) of the whole stream at the final rate, and with need_acc the stage-2 accumulators (ai, aq) and the
    stage-1 intermediates' evidence (part E): rails reached and an accumulator wrapped"""
    shape = cases.shape_of(e)
    if shape not in _REFS:
        d = cases.data(e)
        si, sq = osc(e)
        rows = []
        for c in range(e["channels"]):
            audio, fi, fq = pm.model_q15(orc, d["x"][c], si[c], sq[c], d["p"], e["D1"], d["modes"][c], d["ti"][c], d["tq"][c], e["D2"])
            rows.append(dict(audio=audio, fi=fi, fq=fq))
        _REFS[shape] = rows
    return _REFS[shape]


def stage_one(orc, e, c):
    """(ui, uq, true): the oracle's intermediates of channel c at fs / D1 and the I accumulators before they wrap, at the full rate"""
    d = cases.data(e)
    si, sq = osc(e)
    mi, mq = orc.freqconv_q15(d["x"][c], np.zeros_like(d["x"][c]), si[c], sq[c], 1, 1)
    rc, ui = orc.fir_q15_blocks(d["p"], mi, 128)
    assert rc == 0
    rc, uq = orc.fir_q15_blocks(d["p"], mq, 128)
    assert rc == 0
    true = np.convolve(mi.astype(np.int64), d["p"][::-1].astype(np.int64))[:mi.size]
    return ui[e["D1"] - 1::e["D1"]], uq[e["D1"] - 1::e["D1"]], true


def accs_q15(orc, e):
    """per channel the stage-2 accumulators (ai, aq) behind every output (tests/agc_model.py: arm_fir_fast_q15's before its >> 15)"""
    key = (cases.shape_of(e), "acc")
    if key not in _REFS:
        d = cases.data(e)
        rows = []
        for c, r in enumerate(refs_q15(orc, e)):
            ui, uq, _ = stage_one(orc, e, c)
            ai, aq = agc.acc_q15(ui, d["ti"][c])[e["D2"] - 1::e["D2"]], agc.acc_q15(uq, d["tq"][c])[e["D2"] - 1::e["D2"]]
            assert np.array_equal(agc.plain_q15(ai), r["fi"]) and np.array_equal(agc.plain_q15(aq), r["fq"])          # the two statements of the model agree
            rows.append((ai, aq))
        _REFS[key] = rows
    return _REFS[key]


def gained_q15(orc, e):
    """a gained entry by the model: (audio [ch, outputs], pairs [ch, outputs, 2], records [calls][ch] as msdr_chain_get_agc returns them)"""
    d = cases.data(e)
    acc = accs_q15(orc, e)
    rxs = [agc.Rx() for _ in range(e["channels"])]
    for c, rx in enumerate(rxs):
        rx.set_gain(d["gains"][c])
        rx.on = int(e["agc"])
    total = sum(cases.call_outputs(e))
    audio, pairs, words = np.empty((e["channels"], total), I16), np.empty((e["channels"], total, 2), I16), []
    for s in cases.call_slices(e):
        for c, rx in enumerate(rxs):
            gi, gq = agc.pair_q15(acc[c][0][s], rx.mult), agc.pair_q15(acc[c][1][s], rx.mult)
            pairs[c, s, 0], pairs[c, s, 1] = gi, gq
            audio[c, s] = orc.demod_q15(int(d["modes"][c]), gi, gq)
            rx.after_call(rx.absmax_of(gi, gq))
        words.append([rx.words() for rx in rxs])
    return audio, pairs, words


def expected_q15(orc, e):
    """(audio, pairs, records or None) of the entry"""
    if e["gain"]:
        return gained_q15(orc, e)
    r = refs_q15(orc, e)
    return np.stack([w["audio"] for w in r]), np.stack([np.stack([w["fi"], w["fq"]], axis=1) for w in r]), None


def switch_on(chain, e):
    """the gain of a gained entry: fixed per-channel gains, AGC on every receiver or none"""
    if e["gain"]:
        chain.set_gain(True)
        chain.set_gain_channels(0, cases.data(e)["gains"])
        chain.set_agc(None, int(e["agc"]))


def make_q15(ctx, e, gain=True):
    d = cases.data(e)
    chain = nco_chain(ctx, e["channels"], d["ti"], d["tq"], d["steps"], d["phases"], d["modes"])
    chain.set_prefilter(e["D1"], d["p"])
    chain.set_decimation(e["D2"])
    assert chain.prefilter() == (e["D1"], e["N1"]) and chain.decimation() == e["D2"]
    if gain:
        switch_on(chain, e)
    return chain


def records(chain, e, into):
    """run_entry's hook behind every call: the receivers' records"""
    return (lambda k: into.append([chain.agc_state(c)["words"].copy() for c in range(e["channels"])])) if e["gain"] else None


def part_d(ctx, e, make_plain, call, long_row):
    """one step beyond the limit: the setter refuses with MSDR_STATUS_ARGUMENT_ERROR and the chain is what a control chain that was never asked
    is (test_gpu_decim_census.refusal's comparison: the same decimation, the same bits over 128 samples, the same info()).
    make_plain(nt) -> a chain of nt channel taps in phase-accumulator mode, nothing else set; long_row: a prefilter row of e["refuse"] taps"""
    d = cases.data(e)
    x = d["x"][:, :128]
    if e["limit"] == "taps":          # the row one step longer, asked beside the entry's D2; both chains are then left without prefilter and factor

        def make(nt):
            return make_plain(nt)

        def ask(chain):
            chain.set_decimation(e["D2"])
            try:
                chain.set_prefilter(e["D1"], long_row)
            finally:
                assert chain.prefilter() == (1, 0)
                chain.set_decimation(1)
    else:                             # D2 + 1 behind the entry's prefilter: both chains keep the prefilter and run it at D2 = 1

        def make(nt):
            chain = make_plain(nt)
            chain.set_prefilter(e["D1"], d["p"])
            return chain

        def ask(chain):
            chain.set_decimation(e["refuse"])
    refusal(ctx, dict(e, refuse=e["N2"]), make, call, ask=ask, x=x)


def call_q15(ctx, chain, x):
    D1 = chain.prefilter()[0]
    dy = ctx.array((x.shape[0], x.shape[1] // D1), I16)
    chain.process(ctx.to_device(np.ascontiguousarray(x)), dy, x.shape[1])
    return dy.download()


def plain_q15(ctx, e, nt):
    d = cases.data(e)
    assert nt == e["N2"]
    return nco_chain(ctx, e["channels"], d["ti"], d["tq"], d["steps"], d["phases"], d["modes"])


def rails_and_wrap(orc, e):
    """part E: what the entry itself must show in the reference"""
    seen = dict(high=False, low=False, wrap=False)
    for c in range(e["channels"]):
        ui, _, true = stage_one(orc, e, c)
        seen["high"] |= bool((ui == 32767).any())
        seen["low"] |= bool((ui == -32768).any())
        seen["wrap"] |= bool((np.abs(true[e["D1"] - 1::e["D1"]]) >= 1 << 31).any())
    return seen


@pytest.mark.parametrize("name", cases.names(0))
def test_entry(ctx, orc, name):
    e = cases.BY_NAME[name]
    d = cases.data(e)
    ch = e["channels"]
    want_audio, want_pairs, want_words = expected_q15(orc, e)
    r = refs_q15(orc, e)
    chain = make_q15(ctx, e)
    got_words = []
    audio, pairs, meters = run_entry(ctx, chain, e, I16, I16 if e["iq"] else None, np.uint64 if e["meter"] else None, x=d["x"], calls=cases.call_outputs(e), ran=ran,
                                     read=(0, e["calls"] - 1), after=records(chain, e, got_words), no_audio=not e["out"])
    chain.close()
    for c in range(ch):
        if e["out"]:
            assert np.abs(want_audio[c].astype(np.int32)).max() > 100, c
            assert np.array_equal(audio[c], want_audio[c]), (c, np.flatnonzero(audio[c] != want_audio[c])[:8])
        if e["iq"]:
            assert np.abs(want_pairs[c].astype(np.int32)).max() > 100, c
            assert np.array_equal(pairs[c], want_pairs[c]), (c, np.argwhere(pairs[c] != want_pairs[c])[:8])
        if e["meter"]:          # the meter keeps the ungained pair
            expect = np.array([sums(r[c]["fi"][s], r[c]["fq"][s], s.stop - s.start, s.stop - s.start)[0] for s in cases.call_slices(e)], np.uint64)
            assert np.array_equal(meters[:, c], expect), (c, meters[:, c], expect)
            assert expect.min() > 0
    if e["gain"]:
        for k, (got, want) in enumerate(zip(got_words, want_words)):
            for c in range(ch):
                assert np.array_equal(got[c], want[c]), (k, c, got[c].tolist(), want[c].tolist())
        assert len(got_words) == len(want_words) == e["calls"] and (not e["agc"] or all(w[4] == e["calls"] for w in want_words[-1]))
        assert not np.array_equal(want_audio, np.stack([w["audio"] for w in r]))
    if e["full"] and e["out"] and not e["gain"]:          # the tap and the meter disturb nothing: the same calls on the plain kernel give the same bits
        off = make_q15(ctx, e)
        plain, _, _ = run_entry(ctx, off, e, I16, x=d["x"], calls=cases.call_outputs(e), ran=ran, read=(0, e["calls"] - 1))
        off.close()
        assert np.array_equal(audio, plain)
    if e["kind"] == "sat":
        seen = rails_and_wrap(orc, e)
        assert all(seen.values()), ("the entry must reach both rails and wrap an accumulator", seen)
    if e["part"] == "D":
        long_row = np.concatenate([np.full(e["refuse"] - e["N1"], 7, I16), d["p"]]) if e["limit"] == "taps" else None
        part_d(ctx, e, lambda nt: plain_q15(ctx, e, nt), lambda chain, x: call_q15(ctx, chain, x), long_row)
    assert raw(audio).shape == (ch, sum(cases.call_outputs(e)))
