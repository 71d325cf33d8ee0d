"""The census of the sliding-window per-receiver chain kernels, Q15 half: one case per Q15 entry of tests/pc_census_cases.py -- every launch geometry
pc_geometry can hand chain_q15pc_kernel (chain, both mixers, and FIR stage), chain_q15pco_kernel and chain_q15pcn_kernel, every CPW instantiation
of their metered, I/Q and I/Q-plus-meter twins, an input map, the tap counts around a step of 8, the longest filters the setters accept and time
segments beside fewer than four waves, and the long filters again behind a call that fills their history -- each held to the oracle and to the
memory around its buffers.

Every entry runs the same recipe (the table's docstring; the decimation census's at D = 1): CPW * waves + 1 channels of mixed modes, three calls
over one stream from the zero state -- the entry's length, 2 samples, the entry's length again; part F: a call of np + 1 samples before them --
with audio, pairs and meter of every call in buffers filled with a sentinel between guard stretches (run_entry of
tests/test_gpu_decim_census.py).

References and judges are the existing ones, everything int16 / uint64 and exact: orclib.Oracle.chain_q15 one 128-sample block at a time over the
stream padded with zeros (oracle_row of tests/test_gpu_osc_per_channel.py; the Fs/4 rows with the oracle's own Fs/4 mixer), the phase oscillator
from msdr.nco_q15 as Bank of tests/test_gpu_nco_per_channel.py computes it, pairs from want_iq=True, the meter from sums of
tests/test_gpu_meter_per_channel.py, the FIR stage from fir_expect of tests/test_gpu_taps_per_channel.py.  WHICH code ran is read from
chain.info() after the first and the third call of the entry's length: the family's kernel name, block == 64 waves, tile == 512 / CPW,
lds_bytes == the rule's figure and the number of time segments.  The Q15 twins have no flavour word: that the tap's or the meter's buffer was written with the oracle's
values, and nothing around it, is the evidence.  The FIR stage (msdr_fir_q15, set_coeffs_channels) has no info call: for its entries the evidence
is the oracle and the guards alone."""
import numpy as np
import pytest

import pc_census_cases as cases
from gpuhelp import ctx, msdr  # noqa: F401
from test_gpu_decim_census import refusal, run_entry
from test_gpu_decim_per_channel import nco_chain
from test_gpu_meter_per_channel import padded, sums
from test_gpu_osc_per_channel import oracle_row
from test_gpu_taps_per_channel import fir_expect

pytestmark = pytest.mark.gpu
JUNK = 0x5A5A          # what the input buffer holds behind the antenna rows of an input map
_REFS = {}


def ran(info, e):
    """which code ran, from chain.info() alone"""
    assert info["kernel"].startswith(cases.kernel_name(e["fam"], "")), info
    assert info["block"] == 64 * e["nw"] and info["tile"] == 512 // e["cpw"] == e["tile"], (info, e)
    assert info["lds_bytes"] == e["lds"] and info["time_segments"] == e["nseg"], (info, e)


def antenna(e, x=None):
    """(the stream that is uploaded, feed of run_entry): with an input map the two antenna rows at the start of a buffer of the replicated size.
    x: a stream in place of the entry's own -- [channels, total], or [channels, total, 2] pairs (tests/cx_census_cases.py): the antenna rows
    are then rows of pairs, with the same junk behind them"""
    x = cases.data(e)["x"] if x is None else x
    if not e["inmap"]:
        return x, None

    def feed(part):
        full = np.full((e["channels"],) + part.shape[1:], JUNK, part.dtype)
        full.reshape(-1)[:part.size] = part.reshape(-1)
        return full
    return x[:2], feed


def run_pc(ctx, chain, e, adtype, pdtype=None, mdtype=None, flavour=None, replicated=False, x=None):
    """the entry's calls through run_entry; replicated: every channel's own row is uploaded (the chain has no input map); x: as antenna's"""
    if replicated:
        x, feed = (cases.heard(e) if x is None else x[np.arange(e["channels"]) % 2] if e["inmap"] else x), None
    else:
        x, feed = antenna(e, x)
    return run_entry(ctx, chain, e, adtype, pdtype, mdtype, flavour, x=x, calls=cases.calls(e), ran=ran if e["chain"] else None, feed=feed, read=cases.read_at(e))


# ---- the oracle rows, once per shape --------------------------------------------------------------------------------------------------------
def refs_q15(orc, e):
    """per channel (audio, i, q) of the whole stream (padded with zeros to whole 128-sample blocks); the FIR stage: (output,)"""
    shape = cases.shape_of(e)
    if shape not in _REFS:
        d, x = cases.data(e), cases.heard(e)
        n128 = (d["n"] + 127) // 128 * 128
        if not e["chain"]:
            _REFS[shape] = [(fir_expect(orc, [(0, d["ti"][c])], x[c], 128),) for c in range(e["channels"])]
        elif e["mixer"] == "fs4":
            _REFS[shape] = [orc.chain_q15(padded(x[c], n128), int(d["modes"][c]), d["ti"][c], d["tq"][c], want_iq=True) for c in range(e["channels"])]
        else:
            si, sq = cases.oscillator(e, n128)
            _REFS[shape] = [oracle_row(orc, padded(x[c], n128), si[c], sq[c], lambda b: (d["modes"][c], d["ti"][c], d["tq"][c]), {}, want_iq=True)
                            for c in range(e["channels"])]
    return _REFS[shape]


def make_q15(ctx, e, nt=None, before=False, inmap=None):
    """the entry's chain; nt: with designed rows of nt taps (part D's refusal); before: in the state before the family's last setter"""
    d, ch = cases.data(e), e["channels"]
    if nt is None:
        ti, tq = d["ti"], d["tq"]
    else:
        ti = tq = np.stack([cases.bw_taps(0, 500.0 + 350.0 * c, nt) for c in range(ch)])
    if e["mixer"] == "nco" and not before:
        chain = nco_chain(ctx, ch, ti, tq, d["steps"], d["phases"], d["modes"])
    else:
        if e["mixer"] == "fs4":
            chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, ti[0], tq[0], modes=d["modes"])
        else:
            oi, oq = (d["oi"], d["oq"]) if d["oi"] is not None else cases.osc_rows(1, cases.ROW_LEN, seed=3)
            chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, ti[0], tq[0], mixer=msdr.MIXER_NCO, modes=d["modes"], osc_i=oi[0], osc_q=oq[0])
        chain.set_taps_channels(0, ti, tq)
        if e["mixer"] == "rows" and not before:
            chain.set_osc_channels(0, d["oi"], d["oq"])
    if e["inmap"] if inmap is None else inmap:
        chain.set_input_rows(np.arange(ch) % 2, 2)
    return chain


def ask_q15(e):
    """the setter that refuses the filter one step beyond the family's limit"""
    d = cases.data(e)
    if e["mixer"] == "rows":
        return lambda chain: chain.set_osc_channels(0, d["oi"], d["oq"])
    return lambda chain: chain.set_nco_channels(0, d["steps"].astype(np.uint32), d["phases"].astype(np.uint32))


def call_q15(ctx, chain, x):
    dy = ctx.array(x.shape, np.int16)
    chain.process(ctx.to_device(np.ascontiguousarray(x)), dy, x.shape[1])
    return dy.download()


def fir_entry(ctx, orc, e):
    """the arm_fir_fast_q15 stage with per-channel coefficients: chain_q15pc_kernel<CPW, true>"""
    d, ch, m = cases.data(e), e["channels"], cases.total(e)
    want = refs_q15(orc, e)
    fir = msdr.FirQ15(ctx, d["ti"][0], ch)
    fir.set_coeffs_channels(0, d["ti"])
    got, _, _ = run_pc(ctx, fir, e, np.int16)
    fir.close()
    for c in range(ch):
        w = want[c][0][:m]
        assert np.abs(w.astype(np.int32)).max() > 100, c
        assert np.array_equal(got[c], w), (c, np.flatnonzero(got[c] != w)[:8])


@pytest.mark.parametrize("name", cases.names(0))
def test_entry(ctx, orc, name):
    e = cases.BY_NAME[name]
    if not e["chain"]:
        fir_entry(ctx, orc, e)
        return
    ch, m = e["channels"], cases.total(e)
    meter, iq = "meter" in e["twin"], "iq" in e["twin"]
    want = refs_q15(orc, e)
    chain = make_q15(ctx, e)
    audio, pairs, meters = run_pc(ctx, chain, e, np.int16, np.int16 if iq else None, np.uint64 if meter else None)
    chain.close()
    for c in range(ch):
        w, i, q = (r[:m] for r in want[c])
        assert np.abs(w.astype(np.int32)).max() > 100, c
        assert np.array_equal(audio[c], w), (c, np.flatnonzero(audio[c] != w)[:8])
        if iq:
            assert np.array_equal(pairs[c], np.stack([i, q], axis=1)), c
        if meter:
            lo, expect = 0, []
            for n in cases.calls(e):
                expect.append(sums(i[lo:lo + n], q[lo:lo + n], n, n)[0])
                lo += n
            assert np.array_equal(meters[:, c], np.array(expect, np.uint64)), (c, meters[:, c], expect)
            assert min(expect) > 0
    if e["twin"]:          # the tap and the meter disturb nothing: the same calls on a chain without them give the same bits
        off = make_q15(ctx, e)
        plain, _, _ = run_pc(ctx, off, e, np.int16)
        off.close()
        assert np.array_equal(audio, plain)
    if meter and iq:       # ... and the tap does not disturb the meter
        alone = make_q15(ctx, e)
        _, _, only = run_pc(ctx, alone, e, np.int16, None, np.uint64)
        alone.close()
        assert np.array_equal(meters, only)
    if e["inmap"]:         # the same chain without the map, fed the replicated rows
        twin = make_q15(ctx, e, inmap=False)
        rep, _, _ = run_pc(ctx, twin, e, np.int16, replicated=True)
        twin.close()
        assert np.array_equal(audio, rep)
    if e["refuse"] is not None:
        refusal(ctx, e, lambda nt: make_q15(ctx, e, nt, before=True), lambda chain, x: call_q15(ctx, chain, x), ask=ask_q15(e), x=cases.heard(e)[:, :128])
