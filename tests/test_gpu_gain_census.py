"""The census of the gain twins, Q15 half: one case per Q15 entry of tests/gain_census_cases.py -- every launch geometry pc_geometry and
dec_geometry can hand chain_q15pcn[_cx]_gain_kernel<CPW> and chain_q15pcnd[_cx]_gain_kernel<CPW, AL> (30 instantiations), the superset's
run-time switches in every combination, I/Q-only calls, the arithmetic's corners, the peak's boundary in every instantiation, the longest
filters, time segments beside fewer than four waves and behind a decimator, and agc_step_kernel's second and third workgroup.

Every entry runs the recipe of the other censuses (tests/test_gpu_decim_census.py::run_entry, with this table's stream and calls): three calls
over one stream from the zero state -- the entry's length, 2 outputs, the entry's length again --, audio, pairs and meter of every call in
buffers filled with a sentinel between guard stretches, the receivers' records read behind every call.

Everything is bit for bit (np.array_equal) against tests/agc_model.py::BankQ15 (pinned to the oracle by tests/test_agc_model.py), real input and
complex input with either direction: the audio, the GAINED pairs, the UNGAINED meter sums, and behind every call all 32 words of every
receiver's record -- multiplier, agc_idx, AGC_val, absmax, steps, the ring.  In parts D and F the absmax is the boundary's test: the model's
peak over the same stream followed by zeros to the tile's end is more than four times the call's (tests/test_gain_census_cases.py shows it
without a GPU), so a kernel that counted outputs past n_out would fail the records of the last call.
  which code  chain.info(): the plain kernel's stem (the names stay under msdr_chain_set_gain), block == 64 waves, tile, lds_bytes == the rule's
              figure, time_segments == the rule's count.  The Q15 chains have no flavour word: the evidence that the twin ran is gain() is True,
              complex_input() == (cx, dir), the records, and output bits no plain kernel produces (the model's, under gains other than 1).
  identity    LSB / USB audio is the oracle's demodulator over the STORED pairs, bit for bit, wherever audio and pairs both exist."""
import copy

import numpy as np
import pytest

import agc_model as M
import gain_census_cases as cases
import test_gpu_pc_census as pq
from gpuhelp import ctx, msdr  # noqa: F401
from test_gpu_decim_census import run_entry
from test_gpu_decim_per_channel import nco_chain
from test_gpu_nco_per_channel import Bank

pytestmark = pytest.mark.gpu
I16, U64 = np.int16, np.uint64
_BANKS = {}


def ran(info, e):
    """which code ran, from chain.info() alone"""
    assert info["kernel"].startswith(cases.stem(e)), info
    assert info["block"] == 64 * e["nw"] and info["tile"] == e["tile"], (info, e)
    assert info["lds_bytes"] == e["lds"] and info["time_segments"] == e["nseg"], (info, e)


def streams(e):
    """(xi, xq or None, si, sq): what every receiver hears and its oscillator, [channels, total + pad], zeros behind the stream"""
    d, m = cases.data(e), cases.total(e) + cases.pad(e)
    grow = lambda x: np.concatenate([x, np.zeros((x.shape[0], m - x.shape[1]), x.dtype)], axis=1)          # noqa: E731
    si, sq = Bank(d["steps"], d["phases"]).advance(m)
    return grow(cases.heard(e, d["x"])), (grow(cases.heard(e, d["xq"])) if e["cx"] else None), si, sq


def fresh(proto, e, f32=False):
    """the cached bank with new records under the entry's gains and switches"""
    bank = copy.copy(proto)
    bank.rx = [M.Rx(f32=f32) for _ in range(e["channels"])]
    for c, rx in enumerate(bank.rx):
        rx.set_gain(e["gains"][c])
        rx.on = int(e["agc"][c])
    return bank


def bank_q15(orc, e):
    key = (cases.shape_of(e), e["cx"], e["dir"])
    if key not in _BANKS:
        d = cases.data(e)
        xi, xq, si, sq = streams(e)
        _BANKS[key] = M.BankQ15(orc, xi, xq, si, sq, d["modes"], d["ti"], d["tq"], direction=e["dir"])
    return fresh(_BANKS[key], e)


def spans(e):
    """per call (lo, hi) in input samples"""
    out, lo = [], 0
    for m in cases.calls(e):
        out.append((lo, lo + m * cases.factor(e)))
        lo = out[-1][1]
    return out


def model_q15(orc, e):
    """the entry by the model: audio [ch, outputs], pairs [ch, outputs, 2], meters [calls, ch], words [1 + calls][ch] (before the first call
    and behind every call), and of the last call per receiver `true` (its absmax) and `longer` (with the outputs to the tile's end counted)"""
    bank = bank_q15(orc, e)
    D = cases.factor(e)
    audio, pairs, meters, words = [], [], [], [[rx.words() for rx in bank.rx]]
    for lo, hi in spans(e):
        mults = [rx.mult for rx in bank.rx]
        a, p, s = bank.call(lo, hi, D)
        audio.append(a); pairs.append(p); meters.append(s)
        words.append([rx.words() for rx in bank.rx])
    idx = M.out_index(lo, hi + cases.pad(e), D)
    longer = [bank.rx[c].absmax_of(M.pair_q15(bank.acc[c][0][idx], mults[c]), M.pair_q15(bank.acc[c][1][idx], mults[c])) for c in range(e["channels"])]
    return dict(audio=np.concatenate(audio, axis=1), pairs=np.concatenate(pairs, axis=1), meters=np.stack(meters), words=words,
                true=[rx.absmax for rx in bank.rx], longer=longer, bank=bank)


def switch_on(chain, e):
    """complex input, the factor, the gain: fixed per-receiver gains and the receivers' AGC switches"""
    if e["cx"]:
        chain.set_complex_input(True, e["dir"])
    if e["kind"] == "dec":
        chain.set_decimation(e["D"])
    assert chain.complex_input() == (e["cx"], e["dir"]) and chain.decimation() == cases.factor(e)
    chain.set_gain(True)
    chain.set_gain_channels(0, np.asarray(e["gains"], np.float32))
    chain.set_agc(np.asarray(e["agc"], np.int32))
    assert chain.gain() is True
    return chain


def make_q15(ctx, e):
    d, ch = cases.data(e), e["channels"]
    chain = nco_chain(ctx, ch, d["ti"], d["tq"], d["steps"], d["phases"], d["modes"])
    if e["inmap"]:
        chain.set_input_rows(np.arange(ch) % 2, 2)
    return switch_on(chain, e)


def records(chain, e):
    return [chain.agc_state(c)["words"].copy() for c in range(e["channels"])]


def run_gain(ctx, chain, e, adtype, pdtype, mdtype, flavour=None):
    """the entry's calls through run_entry -> (audio, pairs or None, meters or None, records [1 + calls][ch])"""
    d = cases.data(e)
    x, feed = pq.antenna(e, d["pairs"] if e["cx"] else d["x"])
    words = [records(chain, e)]
    got = run_entry(ctx, chain, e, adtype, pdtype if e["iq"] else None, mdtype if e["meter"] else None, flavour, x=x, calls=cases.calls(e), ran=ran, feed=feed,
                    read=(0, 2), after=lambda k: words.append(records(chain, e)), no_audio=not e["out"])
    return got + (words,)


def same_words(got, want, tag):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        for c in range(len(w)):
            assert np.array_equal(g[c], w[c]), (tag, "call %d" % (k - 1), c, g[c].tolist(), w[c].tolist())


@pytest.mark.parametrize("name", cases.names(0))
def test_entry(ctx, orc, name):
    e = cases.BY_NAME[name]
    d, ch = cases.data(e), e["channels"]
    want = model_q15(orc, e)
    chain = make_q15(ctx, e)
    audio, pairs, meters, words = run_gain(ctx, chain, e, I16, I16, U64)
    chain.close()
    for c in range(ch):
        if e["out"]:
            assert np.array_equal(audio[c], want["audio"][c]), (c, np.flatnonzero(audio[c] != want["audio"][c])[:8])
        if e["iq"]:
            assert np.array_equal(pairs[c], want["pairs"][c]), (c, np.argwhere(pairs[c] != want["pairs"][c])[:8])
        if e["meter"]:          # the meter keeps the ungained pair
            assert np.array_equal(meters[:, c], want["meters"][:, c]), (c, meters[:, c], want["meters"][:, c])
        if e["out"] and e["iq"] and d["modes"][c] in (cases.LSB, cases.USB):
            assert np.array_equal(audio[c], orc.demod_q15(int(d["modes"][c]), np.ascontiguousarray(pairs[c, :, 0]), np.ascontiguousarray(pairs[c, :, 1]))), c
    same_words(words, want["words"], name)
    assert all(int(w[4]) == 3 * e["agc"][c] for c, w in enumerate(words[-1]))
