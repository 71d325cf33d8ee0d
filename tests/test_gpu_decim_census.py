"""The census of the decimating per-receiver chain kernels, Q15 half: one case per entry of tests/decim_census_cases.py -- every launch geometry
dec_geometry can hand chain_q15pcnd_kernel (69 keys), every (CPW, AL) instantiation of its metered, I/Q and I/Q-plus-meter twins, the tap counts
around a step of 8 and the longest filters the setter accepts -- each held to the oracle and to the memory around its buffers.

Every entry runs the same recipe (the table's docstring): CPW * waves + 1 channels of mixed modes, three calls over one stream from the zero
state -- the entry's length, 2 outputs, the entry's length again -- with audio, pairs and meter of every call in buffers filled with a sentinel
between guard stretches (guarded_call's layout of tests/test_gpu_decim_per_channel.py).

References and judges are the existing ones, everything int16 / uint64 and exact: orclib.Oracle.chain_q15 at the FULL rate one 128-sample block
at a time (oracle_row, the stream padded with zeros to whole blocks), subsampled at m D + D - 1 of every call; pairs and meter from
want_iq=True and tests/test_gpu_meter_per_channel.py::sums.  WHICH code ran is read from chain.info() after the first and the third call: the
family's kernel name, block == 64 waves, tile == opl * 64 / CPW and lds_bytes == the rule's figure (together they name CPW, waves and outputs
per lane).  The Q15 twins have no flavour word: that the tap's or the meter's buffer was written with the oracle's values, and nothing around
it, is the evidence."""
import numpy as np
import pytest

import decim_census_cases as cases
from gpuhelp import ctx, msdr  # noqa: F401
from test_gpu_decim_per_channel import nco_chain
from test_gpu_iq_per_channel import pitch_of
from test_gpu_meter_per_channel import padded, sums
from test_gpu_nco_per_channel import Bank
from test_gpu_osc_per_channel import oracle_row

pytestmark = pytest.mark.gpu
ARG = msdr.STATUS_ARGUMENT_ERROR
PATTERN = {2: 0x5A5B, 4: 0x7B5A5B5C, 8: 0xA5A5A5A5A5A5A5A5}          # as bits; the float is 1.13e36, the double negative and below 1e-120: no output of these chains
METER_GUARD = 3


def raw(a):
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def fresh(count, dtype):
    size = np.dtype(dtype).itemsize
    return np.full(count, PATTERN[size], {2: np.uint16, 4: np.uint32, 8: np.uint64}[size]).view(dtype)


def untouched(a):
    return bool((raw(a) == PATTERN[a.dtype.itemsize]).all())


def ran(info, e):
    """which code ran, from chain.info() alone"""
    assert info["kernel"].startswith(cases.kernel_name(e["f32"], "")), info
    assert info["block"] == 64 * e["nw"] and info["tile"] == e["opl"] * 64 // e["cpw"] == e["tile"], (info, e)
    assert info["lds_bytes"] == e["lds"], (info, e)


def run_entry(ctx, chain, e, adtype, pdtype=None, mdtype=None, flavour=None, x=None, calls=None, ran=ran, feed=None, read=(0, 2), after=None, no_audio=False):
    """the entry's three calls -> (audio [ch, outputs], pairs [ch, outputs, 2] or None, meters [3, ch] or None); every buffer lies between guard
    stretches of the sentinel, and everything outside the written rows must still hold it.  flavour(info): a check of the family's own.
    The census of the sliding-window kernels (tests/pc_census_cases.py: no "D" in an entry, audio of n samples per row) hands in its own stream
    x, its calls' lengths, its reading of info() (ran; None: an instance without an info call; read: behind which calls) and, for an input map,
    feed(the call's columns of x) -> what is uploaded.  The census of the complex-input twins (tests/cx_census_cases.py) hands in a stream of
    pairs, x [rows, n, 2]: a call's columns are then n pairs per row, and nothing else changes.  The census of the two-stage kernels
    (tests/pre_census_cases.py) reads the receivers' gain records behind every call -- after(k) runs there -- and makes I/Q-only calls
    (no_audio: a null audio pointer; the guarded audio buffer is still made and must stay the sentinel from end to end)."""
    ch, D = e["channels"], e.get("D", 1)
    x = cases.data(e)["x"] if x is None else x
    audio, pairs, meters, lo = [], [], [], 0
    for k, nout in enumerate(cases.call_outputs(e) if calls is None else calls):
        n = nout * D
        guard = 2 * nout + 8                                             # guarded_call: guard rows in front and behind, n - n / D of slack per row
        a_flat = fresh(guard + ch * nout + ch * (n - nout) + guard, adtype)
        a_buf = ctx.to_device(a_flat)
        if pdtype is not None:
            pitch = pitch_of(nout)
            q_guard = 2 * pitch                                          # pairs: two rows in front and behind
            q_buf = ctx.to_device(fresh(2 * (q_guard + ch * pitch + q_guard), pdtype))
            chain.set_iq_out(q_buf.offset(2 * q_guard * np.dtype(pdtype).itemsize), pitch)
        if mdtype is not None:
            m_buf = ctx.to_device(fresh(METER_GUARD + ch + METER_GUARD, mdtype))
            chain.set_meter(m_buf.offset(8 * METER_GUARD))
        part = np.ascontiguousarray(x[:, lo:lo + n])
        chain.process(ctx.to_device(part if feed is None else feed(part)), None if no_audio else a_buf.offset(guard * a_flat.itemsize), n)
        back = a_buf.download()
        assert untouched(back[:guard]) and untouched(back[guard + ch * nout:]), (k, "audio: written outside the batch")
        assert not no_audio or untouched(back), (k, "audio: written by an I/Q-only call")
        audio.append(back[guard:guard + ch * nout].reshape(ch, nout))
        if pdtype is not None:
            back = q_buf.download().reshape(-1, 2)
            assert untouched(back[:q_guard]) and untouched(back[q_guard + ch * pitch:]), (k, "pairs: written outside the rows")
            rows = back[q_guard:q_guard + ch * pitch].reshape(ch, pitch, 2)
            assert untouched(rows[:, nout:]), (k, "pairs past n_out were written")
            pairs.append(rows[:, :nout])
        if mdtype is not None:
            back = m_buf.download()
            assert untouched(back[:METER_GUARD]) and untouched(back[METER_GUARD + ch:]), (k, "meter: written outside the entries")
            meters.append(back[METER_GUARD:METER_GUARD + ch])
        if k in read and ran is not None:
            info = chain.info()
            ran(info, e)
            if flavour is not None:
                flavour(info)
        if after is not None:
            after(k)
        lo += n
    assert lo == x.shape[1]
    if pdtype is not None:
        chain.set_iq_out(None)
    if mdtype is not None:
        chain.set_meter(None)
    return np.concatenate(audio, axis=1), (np.concatenate(pairs, axis=1) if pairs else None), (np.stack(meters) if meters else None)


def refusal(ctx, e, make, run, ask=None, x=None):
    """part D: one step beyond the limit -- a chain of e["refuse"] taps -- the factor is refused with MSDR_STATUS_ARGUMENT_ERROR and the chain
    is what a control chain that was never asked is: the same decimation, the same bits, the same info().  (Beyond 4096 taps the interface
    refuses the filter itself.)  make(nt) -> a chain of nt taps in phase-accumulator mode; run(chain, x) -> its audio of one call.
    The census of the sliding-window kernels asks another setter: ask(chain) makes the call that must be refused (and make(nt) the chain in the
    state before it); x: the 128 samples per row both chains then process.  Under msdr_chain_set_complex_input (tests/cx_census_cases.py: make
    gives a chain with the mode on, x is pairs) the refusal leaves the mode as it was, too."""
    nt = e["refuse"]
    if nt > cases.TAP_CAP:
        with pytest.raises(msdr.MsdrError) as err:
            make(nt)
        assert err.value.status == ARG, err.value
        return
    a, control = make(nt), make(nt)
    with pytest.raises(msdr.MsdrError) as err:
        a.set_decimation(e["D"]) if ask is None else ask(a)
    assert err.value.status == ARG and "nothing changed" in str(err.value), err.value
    assert a.decimation() == control.decimation() == 1 and a.complex_input() == control.complex_input()
    x = cases.data(e)["x"][:, :128] if x is None else x
    ga, gb = run(a, x), run(control, x)
    assert np.array_equal(raw(ga), raw(gb)) and a.info() == control.info()
    assert "pcnd" not in a.info()["kernel"], a.info()
    a.close()
    control.close()


# ---- the oracle rows, once per shape --------------------------------------------------------------------------------------------------------
_REFS = {}


def refs_q15(orc, e):
    """per channel (audio, i, q) of the whole stream at the full rate (padded with zeros to whole 128-sample blocks)"""
    shape = cases.shape_of(e)
    if shape not in _REFS:
        d = cases.data(e)
        n128 = (d["n"] + 127) // 128 * 128
        si, sq = Bank(d["steps"], d["phases"]).advance(n128)
        _REFS[shape] = [oracle_row(orc, padded(d["x"][c], n128), si[c], sq[c], lambda b: (d["modes"][c], d["ti"][c], d["tq"][c]), {}, want_iq=True)
                        for c in range(e["channels"])]
    return _REFS[shape]


def make_q15(ctx, e, nt=None):
    d = cases.data(e)
    ch = e["channels"]
    if nt is None:
        ti, tq = d["ti"], d["tq"]
    else:
        ti = tq = np.stack([cases.bw_taps(0, 500.0 + 350.0 * c, nt) for c in range(ch)])
    return nco_chain(ctx, ch, ti, tq, d["steps"], d["phases"], d["modes"])


def call_q15(ctx, chain, x):
    dy = ctx.array(x.shape, np.int16)
    chain.process(ctx.to_device(np.ascontiguousarray(x)), dy, x.shape[1])
    return dy.download()


@pytest.mark.parametrize("name", cases.names(0))
def test_entry(ctx, orc, name):
    e = cases.BY_NAME[name]
    ch, D = e["channels"], e["D"]
    meter, iq = "meter" in e["twin"], "iq" in e["twin"]
    want = refs_q15(orc, e)
    idx = cases.out_index(e)
    chain = make_q15(ctx, e)
    chain.set_decimation(D)
    assert chain.decimation() == D
    audio, pairs, meters = run_entry(ctx, chain, e, np.int16, np.int16 if iq else None, np.uint64 if meter else None)
    chain.close()
    for c in range(ch):
        w, i, q = want[c]
        assert np.abs(w[idx].astype(np.int32)).max() > 100, c
        assert np.array_equal(audio[c], w[idx]), (c, np.flatnonzero(audio[c] != w[idx])[:8])
        if iq:
            assert np.array_equal(pairs[c], np.stack([i[idx], q[idx]], axis=1)), c
        if meter:
            lo, expect = 0, []
            for nout in cases.call_outputs(e):
                n = nout * D
                expect.append(sums(i[lo:lo + n], q[lo:lo + n], n, n, D)[0])
                lo += n
            assert np.array_equal(meters[:, c], np.array(expect, np.uint64)), (c, meters[:, c], expect)
            assert min(expect) > 0
    if e["twin"]:          # the tap and the meter disturb nothing: the same calls on a chain without them give the same bits
        off = make_q15(ctx, e)
        off.set_decimation(D)
        plain, _, _ = run_entry(ctx, off, e, np.int16)
        off.close()
        assert np.array_equal(audio, plain)
    if e["part"] == "D":
        refusal(ctx, e, lambda nt: make_q15(ctx, e, nt), lambda chain, x: call_q15(ctx, chain, x))
