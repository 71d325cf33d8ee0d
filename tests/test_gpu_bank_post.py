"""Synchronous AM and the LMS filter for the down-converter bank, Q15 (msdr_chain_set_bank_post): with the switch on a chain created with
MSDR_CHAIN_SYNCAM_PLL and with LMS channels on decimates, and its PLL runs behind the per-receiver kernel on the pairs the kernel's I/Q twin
stores (bank_pll_q15_kernel), at fs / D.  Everything is int16 and bit-exact: np.array_equal, no tolerance.

The oracle per receiver is the existing composition (tests/cx_cases.py: compose_q15 -- msdr_nco_q15 oscillator, freq_conv's mix, the
arm_fir_fast_q15 pair at the full rate; real input is its "Q = 0, dir = 1" form, bit for bit), the pair subsampled at m D + D - 1,
orc_syncam_q15 over the subsampled pair with ONE state across the calls, orc_anr_q15, orc_biquad_teensy_update.

One shape for every case: 70 receivers (one full workgroup of the PLL kernel and a tail of 6) on ONE antenna row, modes cycling AM / SYNCAM /
USB / LSB / CW, LMS off / notch / noise reduction across channels, 102 taps, random oscillator steps with an AM carrier 60 Hz above every
SYNCAM receiver's tuning, three calls of 200, 8 and 130 outputs (across a slab boundary of the PLL kernel, shorter than a slab, even where
nodes need it).  The full-rate pairs are computed once per input kind and shared."""
import numpy as np
import pytest

import orclib
import pll_model
from cx_cases import compose_q15, interleave
from gpuhelp import ctx, msdr  # noqa: F401
from test_gpu_nco_per_channel import Bank, any_table, u32
from test_gpu_osc_per_channel import bw_taps, lowpass, notch, pad

pytestmark = pytest.mark.gpu
FS = 24000.0
CH, NT = 70, 102
NOUTS = (200, 8, 130)
TOTAL = sum(NOUTS)
DMAX = 8
AM, LSB, USB, CW, SYNCAM = orclib.AM, orclib.LSB, orclib.USB, orclib.CW, orclib.SYNCAM
ARG = msdr.STATUS_ARGUMENT_ERROR
PITCH = 216          # the caller's I/Q rows: a multiple of 8 beyond the longest call's 200 pairs
SENT = 0x5A5B
BANK, OLD = "bank_pll_q15_kernel", "syncam_pll_kernel"


@pytest.fixture(scope="module")
def ref(orc, golden):
    """the bank, the antenna row and every receiver's full-rate (audio, I, Q), real and complex input"""
    rng = np.random.default_rng(7100)
    modes = np.array([(AM, SYNCAM, USB, LSB, CW)[c % 5] for c in range(CH)], np.int32)
    anr = np.array([c % 3 for c in range(CH)], np.int32)
    ti = np.stack([bw_taps(1500.0 + 20.0 * c) if modes[c] in (AM, SYNCAM) else pad(golden["taps/FIR_CW_I_coeffs" if modes[c] == CW else "taps/FIR_SSB_I_coeffs"]) for c in range(CH)])
    tq = np.stack([ti[c] if modes[c] in (AM, SYNCAM) else pad(golden["taps/FIR_CW_Q_coeffs" if modes[c] == CW else "taps/FIR_SSB_Q_coeffs"]) for c in range(CH)])
    steps = rng.integers(1, 1 << 32, CH, dtype=np.uint64) | np.uint64(1)
    sync = np.flatnonzero(modes == SYNCAM)
    # the SYNCAM receivers 700 Hz apart from 500 Hz on (off the 128 grid by the odd step), a carrier 60 Hz above each
    steps[sync] = np.array([msdr.nco_step(500.0 + 700.0 * k, FS) for k in range(sync.size)], np.uint64) | np.uint64(1)
    phases = rng.integers(0, 1 << 32, CH, dtype=np.uint64)
    n = TOTAL * DMAX
    n128 = (n + 127) // 128 * 128
    t = np.arange(n128)
    f_rx = steps[sync].astype(np.float64) / 2.0 ** 32 * FS
    carriers = sum((1 + 0.4 * np.sin(2 * np.pi * (150.0 + 11.0 * k) * t / FS)) * np.cos(2 * np.pi * (f + 60.0) * t / FS + 0.3 * k) for k, f in enumerate(f_rx))
    xi = np.round(1400.0 * carriers + rng.normal(0, 150, n128)).astype(np.int16)
    xq = np.round(1400.0 * sum((1 + 0.4 * np.sin(2 * np.pi * (150.0 + 11.0 * k) * t / FS)) * np.sin(2 * np.pi * (f + 60.0) * t / FS + 0.3 * k)
                               for k, f in enumerate(f_rx)) + rng.normal(0, 150, n128)).astype(np.int16)
    si, sq = Bank(steps, phases).advance(n128)
    zero = np.zeros(n128, np.int16)
    # real input: Q = 0, dir = 1; complex input: dir = 0, the spectrum moves down by the receiver's frequency
    full = {kind: [compose_q15(orc, xi, zero if kind == "real" else xq, si[c], sq[c], 1 if kind == "real" else 0, modes[c], ti[c], tq[c])[:3] for c in range(CH)]
            for kind in ("real", "cx")}
    return dict(modes=modes, anr=anr, ti=ti, tq=tq, steps=steps, phases=phases, xi=xi, xq=xq, full=full, sync=sync)


def node_coefs(c, D):
    """two one-stage nodes of the channel's own, designed at the cadence they run at"""
    return lowpass(), notch(c)


def expected(orc, ref, D, kind="real", modes=None, nodes=False, gained=(), k=None):
    """-> (audio [CH, TOTAL], pairs [CH, TOTAL, 2], pll states after every call [calls][CH][3]); k: PLL constants (tests/pll_model.py), None = the oracle's"""
    modes = ref["modes"] if modes is None else modes
    idx = np.arange(D - 1, TOTAL * D, D)
    audio, pairs = np.empty((CH, TOTAL), np.int16), np.empty((CH, TOTAL, 2), np.int16)
    states = [np.zeros((CH, 3), np.float32) for _ in NOUTS]
    for c in range(CH):
        a, fi, fq = (v[idx] for v in ref["full"][kind][c])
        if c in gained:          # gain 0.25: ssat16((acc * 16384) >> 31) = acc >> 17 = (acc >> 15) >> 2 while nothing saturates
            assert np.abs(fi.astype(np.int32)).max() < 32767 and np.abs(fq.astype(np.int32)).max() < 32767
            fi, fq = fi >> 2, fq >> 2
        pairs[c, :, 0], pairs[c, :, 1] = fi, fq
        if modes[c] != ref["modes"][c]:          # (the early-return case moves a SYNCAM channel to AM: the envelope of the same pair)
            a = orc.demod_q15(int(modes[c]), fi, fq)
        pll = orc.syncam_new() if k is None else pll_model.Pll(k)
        lms = orc.anr_new()
        bq = [orc.biquad_teensy_new([co]) for co in node_coefs(c, D)] if nodes else []
        lo = 0
        for call, nout in enumerate(NOUTS):
            seg = a[lo:lo + nout].copy()
            if modes[c] == SYNCAM:
                seg = orc.syncam_q15(pll, fi[lo:lo + nout], fq[lo:lo + nout]) if k is None else pll.run_q15(fi[lo:lo + nout], fq[lo:lo + nout])
                states[call][c] = [pll.fil_out, pll.omega2, pll.phzerror] if k is None else pll.state()
            if ref["anr"][c]:
                seg = orc.anr_q15(lms, int(ref["anr"][c]), seg)
            for b in bq:
                seg = orc.biquad_teensy_update(b, seg)
            audio[c, lo:lo + nout] = seg
            lo += nout
    return audio, pairs, states


def make_chain(ctx, ref, D, kind="real", modes=None, nodes=False, switch=True, anr=True):
    modes = ref["modes"] if modes is None else modes
    kw = dict(biquad_nodes=[[lowpass()], [lowpass()]]) if nodes else {}
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, CH, ref["ti"][0], ref["tq"][0], mixer=msdr.MIXER_NCO, modes=modes, flags=msdr.CHAIN_SYNCAM_PLL, **any_table(), **kw)
    if switch:
        assert not chain.bank_post()
        chain.set_bank_post(True)
        assert chain.bank_post()
    chain.set_taps_channels(0, ref["ti"], ref["tq"])
    chain.set_nco_channels(0, u32(ref["steps"]), u32(ref["phases"]))
    chain.set_input_rows(np.zeros(CH, np.int64), 1)
    if kind == "cx":
        chain.set_complex_input(True, 0)
    if nodes:
        chain.set_node_coefficients_channels(0, 0, 0, np.stack([node_coefs(c, D)[0] for c in range(CH)]))
        chain.set_node_coefficients_channels(1, 0, 0, np.stack([node_coefs(c, D)[1] for c in range(CH)]))
    if anr:
        chain.set_anr(ref["anr"])
    if D > 1:
        chain.set_decimation(D)
    return chain


def run_calls(ctx, chain, ref, D, kind="real", iq_buf=False):
    """the three calls into guarded buffers -> (audio, pairs or None, pll states after every call, post_kernel() after every call)"""
    x = interleave(ref["xi"], ref["xq"])[None] if kind == "cx" else ref["xi"][None]
    audio, pairs = np.empty((CH, TOTAL), np.int16), np.empty((CH, TOTAL, 2), np.int16) if iq_buf else None
    states, names = [], []
    guard = 2 * PITCH
    if iq_buf:
        fresh = np.full((CH + 2) * PITCH * 2 + 16, SENT, np.uint16).view(np.int16)
        buf = ctx.to_device(fresh)
        chain.set_iq_out(buf.offset(PITCH * 4), PITCH)
    lo = 0
    for nout in NOUTS:
        flat = np.full(guard + CH * nout + guard, SENT, np.uint16).view(np.int16)
        dy = ctx.to_device(flat)
        if iq_buf:
            buf.upload(fresh)
        chain.process(ctx.to_device(np.ascontiguousarray(x[:, lo * D:(lo + nout) * D])), dy.offset(guard * 2), nout * D)
        back = dy.download()
        assert (back[:guard].view(np.uint16) == SENT).all() and (back[guard + CH * nout:].view(np.uint16) == SENT).all(), ("audio guard rows", nout)
        audio[:, lo:lo + nout] = back[guard:guard + CH * nout].reshape(CH, nout)
        if iq_buf:
            pb = buf.download().view(np.uint16)
            rows = pb[PITCH * 2:(CH + 1) * PITCH * 2].reshape(CH, PITCH, 2)
            assert (pb[:PITCH * 2] == SENT).all() and (pb[(CH + 1) * PITCH * 2:] == SENT).all() and (rows[:, nout:] == SENT).all(), ("pair guard rows", nout)
            pairs[:, lo:lo + nout] = rows[:, :nout].view(np.int16)
        states.append(np.stack([chain.pll_state(c) for c in ref["sync"]]))
        names.append(chain.post_kernel())
        lo += nout
    return audio, pairs, states, names


def same_states(ref, got, want, tag):
    for call in range(len(NOUTS)):
        w = np.stack([want[call][c] for c in ref["sync"]])
        assert np.array_equal(got[call].view(np.uint32), w.view(np.uint32)), (tag, call)


@pytest.mark.parametrize("iq_buf", [False, True])
@pytest.mark.parametrize("nodes", [False, True])
@pytest.mark.parametrize("D", [1, 3, 8])
def test_audio_pairs_and_pll_state_equal_the_oracle(ctx, orc, ref, D, nodes, iq_buf):
    want_audio, want_pairs, want_states = expected(orc, ref, D, nodes=nodes)
    chain = make_chain(ctx, ref, D, nodes=nodes)
    audio, pairs, states, names = run_calls(ctx, chain, ref, D, iq_buf=iq_buf)
    assert names == [BANK] * 3, names          # the documented rule: every audio call of a chain with the switch on while a channel is on SYNCAM
    assert chain.info()["kernel"].startswith("chain_q15pcnd_kernel" if D > 1 else "chain_q15pcn_kernel"), chain.info()
    bad = [c for c in range(CH) if not np.array_equal(audio[c], want_audio[c])]
    assert not bad, (D, nodes, iq_buf, bad)
    if iq_buf:
        assert np.array_equal(pairs, want_pairs)
    same_states(ref, states, want_states, (D, nodes, iq_buf))
    assert np.abs(want_audio[ref["sync"]].astype(np.int32)).max() > 500 and all(s.any() for s in states)
    chain.close()


def test_a_workgroup_without_a_syncam_channel_leaves_its_rows_alone(ctx, orc, ref):
    """channels 64 .. 69 all off SYNCAM: the PLL kernel's second workgroup returns before its first load"""
    modes = ref["modes"].copy()
    modes[64:][modes[64:] == SYNCAM] = AM
    assert (modes[64:] != SYNCAM).all() and (modes[:64] == SYNCAM).sum() == 13
    want_audio, _, want_states = expected(orc, ref, 3, modes=modes)
    chain = make_chain(ctx, ref, 3, modes=modes)
    audio, _, states, names = run_calls(ctx, chain, ref, 3)
    assert np.array_equal(audio, want_audio) and names == [BANK] * 3
    for call in range(3):
        for k, c in enumerate(ref["sync"]):
            w = want_states[call][c] if c < 64 else np.zeros(3, np.float32)
            assert np.array_equal(states[call][k].view(np.uint32), w.view(np.uint32)), (call, c)
    chain.close()


def test_the_pll_receives_the_gained_pair(ctx, orc, ref):
    g = int(ref["sync"][2])
    want_audio, want_pairs, want_states = expected(orc, ref, 3, gained=(g,))
    chain = make_chain(ctx, ref, 3)
    chain.set_gain(True)
    chain.set_gain_channels(g, np.array([0.25], np.float32))
    audio, pairs, states, _ = run_calls(ctx, chain, ref, 3, iq_buf=True)
    assert np.array_equal(pairs, want_pairs)
    bad = [c for c in range(CH) if not np.array_equal(audio[c], want_audio[c])]
    assert not bad, bad
    same_states(ref, states, want_states, "gain")
    chain.close()


def test_complex_input(ctx, orc, ref):
    want_audio, want_pairs, want_states = expected(orc, ref, 3, kind="cx")
    chain = make_chain(ctx, ref, 3, kind="cx")
    audio, pairs, states, _ = run_calls(ctx, chain, ref, 3, kind="cx", iq_buf=True)
    assert np.array_equal(pairs, want_pairs)
    bad = [c for c in range(CH) if not np.array_equal(audio[c], want_audio[c])]
    assert not bad, bad
    same_states(ref, states, want_states, "cx")
    chain.close()


def test_the_constants_of_the_decimated_rate(ctx, orc, ref):
    """set_pll_rate(fs / 8) at D = 8: tests/pll_model.py with syncam_constants_rate(fs / 8)"""
    D = 8
    k = msdr.syncam_constants_rate(FS / D)
    want_audio, _, want_states = expected(orc, ref, D, k=k)
    chain = make_chain(ctx, ref, D)
    assert chain.pll_rate() == 0.0
    chain.set_pll_rate(FS / D)
    assert chain.pll_rate() == FS / D
    audio, _, states, _ = run_calls(ctx, chain, ref, D)
    bad = [c for c in range(CH) if not np.array_equal(audio[c], want_audio[c])]
    assert not bad, bad
    same_states(ref, states, want_states, "rate")
    ref_audio, _, _ = expected(orc, ref, D)
    assert not np.array_equal(ref_audio, want_audio)          # (the constants matter)
    chain.close()


def test_at_d_one_the_switch_changes_no_bit(ctx, ref):
    outs = []
    for switch in (False, True):
        chain = make_chain(ctx, ref, 1, nodes=True, switch=switch)
        audio, _, states, names = run_calls(ctx, chain, ref, 1)
        assert names == [BANK if switch else OLD] * 3, names
        outs.append((audio, states))
        chain.close()
    assert np.array_equal(outs[0][0], outs[1][0])
    for a, b in zip(outs[0][1], outs[1][1]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_post_kernel_names_the_pll_kernel_of_the_last_audio_call(ctx, ref):
    """"" before the first call and while no channel is on SYNCAM; an I/Q-only call leaves name and PLL state alone"""
    chain = make_chain(ctx, ref, 3)
    assert chain.post_kernel() == ""
    x = ref["xi"][None, :24]
    dy = ctx.array((CH, 8), np.int16)
    chain.process(ctx.to_device(x), dy, 24)
    assert chain.post_kernel() == BANK
    before = np.stack([chain.pll_state(c) for c in ref["sync"]])
    buf = ctx.to_device(np.zeros((CH, 8, 2), np.int16))
    chain.set_iq_out(buf, 8)
    chain.process(ctx.to_device(x), None, 24)
    assert chain.post_kernel() == BANK
    assert np.array_equal(before.view(np.uint32), np.stack([chain.pll_state(c) for c in ref["sync"]]).view(np.uint32))
    for c in ref["sync"]:
        chain.set_mode(int(c), AM)
    chain.process(ctx.to_device(x), dy, 24)
    assert chain.post_kernel() == ""
    for c in ref["sync"]:
        chain.set_mode(int(c), SYNCAM)
    chain.process(ctx.to_device(x), dy, 24)
    before = np.stack([chain.pll_state(c) for c in ref["sync"]])
    chain.init_fir()                                                   # FIR state only: the loops keep theirs
    assert before.any() and np.array_equal(before.view(np.uint32), np.stack([chain.pll_state(c) for c in ref["sync"]]).view(np.uint32))
    chain.reset()
    assert not np.stack([chain.pll_state(c) for c in ref["sync"]]).any()
    chain.close()
