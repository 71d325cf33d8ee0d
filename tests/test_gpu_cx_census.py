"""The census of the complex-input chain kernels, Q15 half: one case per Q15 entry of tests/cx_census_cases.py -- every launch geometry
pc_geometry and dec_geometry can hand chain_q15pcn_cx_kernel<CPW> and chain_q15pcnd_cx_kernel<CPW, AL>, every instantiation of their metered,
I/Q and I/Q-plus-meter twins (60 in all), the input map over rows of pairs, the tap counts, the longest filters, time segments beside fewer than
four waves and the long filters behind a call that fills their history -- each held to the composed oracle and to the memory around its buffers.

Every entry runs its parent's recipe (run_entry of tests/test_gpu_decim_census.py, through run_pc of tests/test_gpu_pc_census.py for the
sliding-window half) on its parent's chain with set_complex_input(True, dir), over rows of pairs {I, Q}: guard stretches of a sentinel around
audio, pairs and meter of every call, chain.info() read behind the first and the third call of the entry's length.

  reference   tests/cx_cases.py's composition of the oracle's own stages, per channel at the full rate over the stream padded with zero pairs to
              whole 128-sample blocks: freqconv_q15 -> fir_q15_blocks pair -> demod_q15, oscillator rows from Bank(steps, phases); decimated
              outputs are those at m D + D - 1 of each call.  Audio and pairs with ==; the meter is the integer sum of fi^2 + fq^2 over each
              call's outputs, with == and above 0.
  which code  the real kernel's stem (the names stay), block == 64 waves, tile, lds_bytes == the rule's figure and the segment count.  The Q15
              chains have no flavour word: the evidence that the twin ran is complex_input() == (True, dir) and output bits that no real-input
              run of the same buffer produces (the oracle's, with a full-scale Q stream mixed in).
  identities  audio with the tap or the meter set is bit-identical to the plain cx chain; the meter beside the tap is the meter alone; an entry
              with an input map is bit-identical to the same chain fed the replicated rows of pairs.
  degenerate  the same chain with dir = 1 over {I, 0} against the REAL chain of the parent entry over I: audio, pairs, meter and history bit for
              bit.  No oracle in it: it ties every cx instantiation to its census-checked real twin.
  history     after the last call fir_history(c) of the first and the last channel is [hist_len, 2] and holds the last hist_len pairs the
              channel heard (zeros in front of the stream): the 2-sample call lies in between, so history_kernel<int32_t> -- with an input
              map history_rows_kernel<int32_t> -- has carried older pairs over.
  part D      the parent's refusal on a chain with the mode on: one step beyond the limit is refused with MSDR_STATUS_ARGUMENT_ERROR, and the
              chain is what a control chain that was never asked is -- the same bits, info() and complex_input()."""
import numpy as np
import pytest

import cx_census_cases as cases
import test_gpu_decim_census as dq
import test_gpu_pc_census as pq
from cx_cases import compose_q15
from gpuhelp import ctx, msdr  # noqa: F401
from test_gpu_decim_census import refusal, run_entry
from test_gpu_meter_per_channel import padded
from test_gpu_nco_per_channel import Bank

pytestmark = pytest.mark.gpu
ARG = msdr.STATUS_ARGUMENT_ERROR
I16, U64 = np.int16, np.uint64
_REFS = {}


# ---- what both arithmetics share ------------------------------------------------------------------------------------------------------------------
def oscillator(e, n):
    """(sin, cos) int16 [channels, n] of the entry's bank over the first n samples"""
    d = cases.data(e)
    return Bank(d["steps"], d["phases"]).advance(n)


def cached(e, kind, build):
    """per channel build(d, xi, xq, si, sq, c) over the stream padded with zero pairs to whole blocks, once per (shape, dir)"""
    k = (cases.shape_of(e), e["dir"], kind)
    if k not in _REFS:
        d = cases.data(e)
        n128 = (d["n"] + 127) // 128 * 128
        si, sq = oscillator(e, n128)
        xi, xq = padded(cases.heard(e, d["x"]), n128), padded(cases.heard(e, d["xq"]), n128)
        _REFS[k] = [build(d, xi[c], xq[c], si[c], sq[c], c) for c in range(e["channels"])]
    return _REFS[k]


def refs_q15(orc, e):
    """per channel (audio, fi, fq, I', Q') int16 at the full rate"""
    return cached(e, "q15", lambda d, xi, xq, si, sq, c: compose_q15(orc, xi, xq, si, sq, e["dir"], d["modes"][c], d["ti"][c], d["tq"][c]))


def with_mode(chain, direction):
    chain.set_complex_input(True, direction)
    assert chain.complex_input() == (True, direction)
    return chain


def run_cx(ctx, chain, e, x, adtype, pdtype=None, mdtype=None, flavour=None, replicated=False):
    """the entry's calls over the stream x ([channels, total, 2] pairs, or [channels, total] on a chain with real input) ->
    (audio, pairs, meters, the history of the first and the last channel behind the last call)"""
    if e["kind"] == "pc":
        got = pq.run_pc(ctx, chain, e, adtype, pdtype, mdtype, flavour, replicated=replicated, x=x)
    else:
        got = run_entry(ctx, chain, e, adtype, pdtype, mdtype, flavour, x=x)
    return got + ([chain.fir_history(c) for c in (0, e["channels"] - 1)],)


def history_is_what_was_heard(e, hist, x, real_len=None):
    """hist: fir_history of the first and the last channel behind the last call; x: the stream of pairs"""
    hear = cases.heard(e, x)
    for h, c in zip(hist, (0, e["channels"] - 1)):
        hl = h.shape[0]
        assert h.shape == (hl, 2) and hl >= ((e["nt"] + 3) & ~3) - 1 and (real_len is None or hl == real_len), (c, h.shape, real_len)
        assert np.array_equal(h, np.concatenate([np.zeros((hl, 2), I16), hear[c]])[-hl:]), (c, "history")


def call(ctx, chain, x, adtype):
    dy = ctx.array(x.shape[:2], adtype)
    chain.process(ctx.to_device(np.ascontiguousarray(x)), dy, x.shape[1])
    return dy.download()


def meter_index(e):
    """per call the input indices of its outputs"""
    idx = cases.out_index(e)
    return [idx[s] for s in cases.call_slices(e)]


# ---- Q15 ------------------------------------------------------------------------------------------------------------------------------------------------
def real_q15(ctx, e, nt=None, inmap=None, decimate=True):
    """the parent entry's chain"""
    if e["kind"] == "pc":
        return pq.make_q15(ctx, e, nt=nt, inmap=inmap)
    chain = dq.make_q15(ctx, e, nt)
    if decimate:
        chain.set_decimation(e["D"])
        assert chain.decimation() == e["D"]
    return chain


def part_d(ctx, e, make, adtype):
    """the parent's refusal on a chain with the mode on; make(nt): the parent's chain of nt taps in the state before the setter that refuses.
    Decimating half: a chain of e["refuse"] taps with complex input, asked for the factor.  Sliding-window half: the setter that refuses is the
    FIRST set_nco_channels, before which the chain has no phase-accumulator oscillator and set_complex_input is itself refused -- both refusals
    leave a real-input chain that equals the control"""
    d = cases.data(e)
    if e["kind"] == "dec":
        def run(chain, x):
            assert chain.complex_input() == (True, e["dir"])
            return call(ctx, chain, x, adtype)
        refusal(ctx, e, lambda nt: with_mode(make(nt), e["dir"]), run, x=d["pairs"][:, :128])
        return

    def run(chain, x):
        with pytest.raises(msdr.MsdrError) as err:
            chain.set_complex_input(True, e["dir"])
        assert err.value.status == ARG and "nothing changed" in str(err.value) and chain.complex_input() == (False, 0), err.value
        return call(ctx, chain, x, adtype)
    ask = lambda chain: chain.set_nco_channels(0, d["steps"].astype(np.uint32), d["phases"].astype(np.uint32))          # noqa: E731
    refusal(ctx, e, make, run, ask=ask, x=cases.heard(e, d["x"])[:, :128])


@pytest.mark.parametrize("name", cases.names(0))
def test_entry(ctx, orc, name):
    e = cases.BY_NAME[name]
    d, ch, idx = cases.data(e), e["channels"], cases.out_index(e)
    meter, iq = "meter" in e["twin"], "iq" in e["twin"]
    want = refs_q15(orc, e)

    def run(direction, x, with_meter=meter, with_iq=iq, inmap=None, replicated=False):
        """direction None: the parent's real chain"""
        chain = real_q15(ctx, e, inmap=inmap)
        if direction is not None:
            with_mode(chain, direction)
        got = run_cx(ctx, chain, e, x, I16, I16 if with_iq else None, U64 if with_meter else None, replicated=replicated)
        chain.close()
        return got

    audio, pairs, meters, hist = run(e["dir"], d["pairs"])
    for c in range(ch):
        w, fi, fq = (r[idx] for r in want[c][:3])
        assert np.abs(w.astype(np.int32)).max() > 100, c
        assert np.array_equal(audio[c], w), (c, np.flatnonzero(audio[c] != w)[:8])
        if iq:
            assert np.array_equal(pairs[c], np.stack([fi, fq], axis=1)), c
        if meter:
            expect = [int((want[c][1][k].astype(np.int64) ** 2 + want[c][2][k].astype(np.int64) ** 2).sum()) for k in meter_index(e)]
            assert np.array_equal(meters[:, c], np.array(expect, U64)), (c, meters[:, c], expect)
            assert min(expect) > 0
    # the degenerate form: dir = 1 over {I, 0} is the parent's real chain over I
    r_audio, r_pairs, r_meters, r_hist = run(None, d["x"])
    z_audio, z_pairs, z_meters, z_hist = run(1, d["pairs_q0"])
    assert np.array_equal(z_audio, r_audio) and np.abs(r_audio.astype(np.int32)).max() > 100
    assert not any(np.array_equal(audio[c], r_audio[c]) for c in range(ch))          # (no flavour word on Q15: the Q stream is in every channel's bits)
    assert (not iq or np.array_equal(z_pairs, r_pairs)) and (not meter or np.array_equal(z_meters, r_meters))
    assert all(zh.shape == rh.shape + (2,) and np.array_equal(zh[:, 0], rh) and not zh[:, 1].any() for zh, rh in zip(z_hist, r_hist))
    history_is_what_was_heard(e, hist, d["pairs"], real_len=r_hist[0].shape[0])
    if e["twin"]:          # the tap and the meter disturb nothing: the same calls on a cx chain without them give the same bits
        plain = run(e["dir"], d["pairs"], False, False)[0]
        assert np.array_equal(audio, plain)
    if meter and iq:       # ... and the tap does not disturb the meter
        only = run(e["dir"], d["pairs"], True, False)[2]
        assert np.array_equal(meters, only)
    if e["inmap"]:         # the same chain without the map, fed the replicated rows of pairs
        rep = run(e["dir"], d["pairs"], inmap=False, replicated=True)
        assert np.array_equal(audio, rep[0])
        history_is_what_was_heard(e, rep[3], d["pairs"])
    if e["refuse"] is not None:
        part_d(ctx, e, lambda nt: pq.make_q15(ctx, e, nt, before=True) if e["kind"] == "pc" else real_q15(ctx, e, nt, decimate=False), I16)
