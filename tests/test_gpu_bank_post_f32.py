"""Synchronous AM and the LMS filter for the down-converter bank, fp32 (msdr_chain_set_bank_post): with the switch on an fp32 chain created
with MSDR_CHAIN_SYNCAM_PLL and / or with LMS channels on enters phase-accumulator mode, and its PLL (bank_pll_f32_kernel) and LMS filter run
behind the per-receiver kernel on the pairs the kernel's I/Q twin stores, at fs / D, in front of the CMSIS-order cascade.

The shape is tests/test_gpu_bank_post.py's (70 receivers on one antenna row, modes cycling AM / SYNCAM / USB / LSB / CW, LMS off / 1 / 2,
102 taps, a carrier 60 Hz above every SYNCAM receiver, calls of 200, 8 and 130 outputs), checked in three parts after the manner of
tests/test_gpu_chain_post.py:
 1. stored pairs against the oracle's (tests/cx_cases.py: compose_f32, subsampled at m D + D - 1): the project's fp32 bound, 1e-5
 2. PLL audio against orc_syncam_f32 applied to the DEVICE's own stored pairs with one state across the calls: the kernel is the oracle's
    statement sequence, so bit-identity -- held to 1e-5 of the pair level where a device sin / cos / atan2 differs from the host's in a last
    place; the figure and the number of differing samples are printed
 3. LMS channels: the filter's arithmetic against orc_anr_f32 applied to the device's audio IN FRONT of the filter, read from a second chain
    with the filter and the cascade off: bit-identical without a cascade, 1e-5 of the level in front of the filter with one (the two-part
    rule; tests/test_gpu_chain_post.py's header says why)."""
import numpy as np
import pytest

import orclib
from cx_cases import compose_f32, interleave
from f32pc_cases import bw_taps, cascade, hilbert_pair
from gpuhelp import ctx, msdr  # noqa: F401
from test_gpu_nco_per_channel import Bank, u32
from test_gpu_nco_per_channel_f32 import any_table, f32

pytestmark = pytest.mark.gpu
FS = 24000.0
CH, NT = 70, 102
NOUTS = (200, 8, 130)
TOTAL = sum(NOUTS)
DMAX = 8
TOL = 1e-5
AM, LSB, USB, CW, SYNCAM = orclib.AM, orclib.LSB, orclib.USB, orclib.CW, orclib.SYNCAM
PITCH = 216
BANK = "bank_pll_f32_kernel"


@pytest.fixture(scope="module")
def ref(orc):
    rng = np.random.default_rng(7200)
    modes = np.array([(AM, SYNCAM, USB, LSB, CW)[c % 5] for c in range(CH)], np.int32)
    anr = np.array([c % 3 for c in range(CH)], np.int32)
    ssb, cw = hilbert_pair(NT), hilbert_pair(NT, 700.0, 300.0)
    ti = np.stack([bw_taps(1500.0 + 20.0 * c) if modes[c] in (AM, SYNCAM) else (cw if modes[c] == CW else ssb)[0] for c in range(CH)])
    tq = np.stack([ti[c] if modes[c] in (AM, SYNCAM) else (cw if modes[c] == CW else ssb)[1] for c in range(CH)])
    steps = rng.integers(1, 1 << 32, CH, dtype=np.uint64) | np.uint64(1)
    sync = np.flatnonzero(modes == SYNCAM)
    steps[sync] = np.array([msdr.nco_step(500.0 + 700.0 * k, FS) for k in range(sync.size)], np.uint64) | np.uint64(1)
    phases = rng.integers(0, 1 << 32, CH, dtype=np.uint64)
    n = TOTAL * DMAX
    n128 = (n + 127) // 128 * 128
    t = np.arange(n128)
    f_rx = steps[sync].astype(np.float64) / 2.0 ** 32 * FS
    env = [1 + 0.4 * np.sin(2 * np.pi * (150.0 + 11.0 * k) * t / FS) for k in range(sync.size)]
    xi = np.round(1400.0 * sum(e * np.cos(2 * np.pi * (f + 60.0) * t / FS + 0.3 * k) for k, (e, f) in enumerate(zip(env, f_rx))) + rng.normal(0, 150, n128)).astype(np.int16)
    xq = np.round(1400.0 * sum(e * np.sin(2 * np.pi * (f + 60.0) * t / FS + 0.3 * k) for k, (e, f) in enumerate(zip(env, f_rx))) + rng.normal(0, 150, n128)).astype(np.int16)
    si, sq = Bank(steps, phases).advance(n128)
    zero = np.zeros(n128, np.int16)
    full = {kind: [compose_f32(orc, xi, zero if kind == "real" else xq, si[c], sq[c], 1 if kind == "real" else 0, modes[c], ti[c], tq[c]) for c in range(CH)]
            for kind in ("real", "cx")}
    rows = np.stack([cascade("lp+notch") * np.float32([1.0, 1.0 - 0.002 * c, 1.0, 1.0 - 0.002 * c, 1.0]) for c in range(CH)])
    return dict(modes=modes, anr=anr, ti=ti, tq=tq, steps=steps, phases=phases, xi=xi, xq=xq, si=si, sq=sq, full=full, sync=sync, rows=rows)


def make_chain(ctx, ref, D, kind="real", lms=True, bq=None, flags=0, switch=True, modes=None, pll=True):
    """bq: None, "shared" (the chain's cascade) or "rows" (per-channel rows behind the PLL)"""
    modes = ref["modes"] if modes is None else modes
    chain = msdr.Chain(ctx, msdr.ARITH_F32, CH, ref["ti"][0], ref["tq"][0], mixer=msdr.MIXER_NCO, modes=modes, biquad_coeffs=cascade("lp+notch") if bq else None,
                       flags=(msdr.CHAIN_SYNCAM_PLL if pll else 0) | flags, **any_table())
    if switch:
        chain.set_bank_post(True)
    chain.set_nco_channels(0, u32(ref["steps"]), u32(ref["phases"]))
    chain.set_taps_channels_f32(0, ref["ti"], ref["tq"])
    chain.set_input_rows(np.zeros(CH, np.int64), 1)
    if kind == "cx":
        chain.set_complex_input(True, 0)
    if bq == "rows":
        chain.set_biquad_coeffs_channels(0, ref["rows"])
    if lms:
        chain.set_anr(ref["anr"])
    if D > 1:
        chain.set_decimation(D)
    return chain


def run_calls(ctx, chain, ref, D, kind="real", iq_buf=True, dtype=np.float32, audio_of=lambda call: True, pll=True):
    """-> (audio [CH, TOTAL], pairs [CH, TOTAL, 2], pll states per call, flavours per call, post_kernel per call); guard rows around both"""
    x = interleave(ref["xi"], ref["xq"])[None] if kind == "cx" else ref["xi"][None]
    audio, pairs = np.zeros((CH, TOTAL), dtype), np.empty((CH, TOTAL, 2), np.float32)
    states, flav, names = [], [], []
    sent = np.float32(1.13e36)
    if iq_buf:
        fresh = np.full((CH + 2) * PITCH * 2 + 16, sent, np.float32)
        buf = ctx.to_device(fresh)
        chain.set_iq_out(buf.offset(PITCH * 8), PITCH)
    lo = 0
    for call, nout in enumerate(NOUTS):
        guard = 2 * PITCH
        flat = np.full(guard + CH * nout + guard, 0x5A5B if dtype == np.int16 else sent, dtype)
        dy = ctx.to_device(flat)
        if iq_buf:
            buf.upload(fresh)
        chain.process(ctx.to_device(np.ascontiguousarray(x[:, lo * D:(lo + nout) * D])), dy.offset(guard * flat.itemsize) if audio_of(call) else None, nout * D)
        back = dy.download()
        assert (back[:guard] == flat[0]).all() and (back[guard + CH * nout:] == flat[0]).all(), ("audio guard rows", nout)
        if audio_of(call):
            audio[:, lo:lo + nout] = back[guard:guard + CH * nout].reshape(CH, nout)
        else:
            assert (back == flat[0]).all()
        if iq_buf:
            pb = buf.download()
            rows = pb[PITCH * 2:(CH + 1) * PITCH * 2].reshape(CH, PITCH, 2)
            assert (pb[:PITCH * 2] == sent).all() and (pb[(CH + 1) * PITCH * 2:] == sent).all() and (rows[:, nout:] == sent).all(), ("pair guard rows", nout)
            pairs[:, lo:lo + nout] = rows[:, :nout]
        states.append(np.stack([chain.pll_state(c) for c in ref["sync"]]) if pll else None)
        flav.append(chain.info()["flavour"])
        names.append(chain.post_kernel())
        lo += nout
    return audio, pairs, states, flav, names


def pair_ratio(pairs, i, q):
    p = pairs.astype(np.float64)
    return float(np.sqrt(((p[:, 0] - i) ** 2 + (p[:, 1] - q) ** 2).sum()) / np.sqrt((i.astype(np.float64) ** 2 + q.astype(np.float64) ** 2).sum()))


def pll_of_pairs(orc, pairs):
    """orc_syncam_f32 over one channel's stored pairs, one state across the calls -> (audio, states per call)"""
    st, out, states, lo = orc.syncam_new(), np.empty(TOTAL, np.float32), [], 0
    for nout in NOUTS:
        out[lo:lo + nout] = orc.syncam_f32(st, pairs[lo:lo + nout, 0], pairs[lo:lo + nout, 1])
        states.append(np.array([st.fil_out, st.omega2, st.phzerror], np.float32))
        lo += nout
    return out, states


def lms_of(orc, on, pre, bq=None):
    """orc_anr_f32 over one channel's audio in front of the filter, one state across the calls, then the cascade from zero state"""
    a, out, lo = orc.anr_new(), np.empty(TOTAL, np.float32), 0
    for nout in NOUTS:
        out[lo:lo + nout] = orc.anr_f32(a, int(on), pre[lo:lo + nout])
        lo += nout
    return out if bq is None else orc.biquad_df1_zero_state(bq, out)


def level(v):
    return float(np.sqrt((v.astype(np.float64) ** 2).sum()))


@pytest.mark.parametrize("D, kind, gain", [(1, "real", False), (3, "real", False), (8, "real", False), (3, "real", True), (3, "cx", False)])
def test_the_three_parts(ctx, orc, ref, D, kind, gain):
    idx = np.arange(D - 1, TOTAL * D, D)
    g = int(ref["sync"][2])
    chains = [make_chain(ctx, ref, D, kind=kind, lms=lms) for lms in (True, False)]          # the chain, and the one with the filter off
    for c in chains:
        if gain:
            c.set_gain(True)
            c.set_gain_channels(g, np.array([0.25], np.float32))
    audio, pairs, states, flav, names = run_calls(ctx, chains[0], ref, D, kind=kind)
    pre, pre_pairs, _, pre_flav, _ = run_calls(ctx, chains[1], ref, D, kind=kind)
    assert names == [BANK] * 3 and all(f & msdr.FLAVOUR_BANK_POST for f in flav + pre_flav), (names, flav)
    assert np.array_equal(pairs.view(np.uint32), pre_pairs.view(np.uint32))
    worst_pair = worst_pll = 0.0
    differing = 0
    for c in range(CH):
        _, fi, fq = (v[idx] for v in ref["full"][kind][c])
        if gain and c == g:
            fi, fq = fi * np.float32(0.25), fq * np.float32(0.25)
        worst_pair = max(worst_pair, pair_ratio(pairs[c], fi, fq))                        # part 1
        if ref["modes"][c] == SYNCAM:                                                      # part 2: the PLL in front of the filter
            want, want_states = pll_of_pairs(orc, pairs[c])
            k = list(ref["sync"]).index(c)
            bits = np.array_equal(pre[c].view(np.uint32), want.view(np.uint32)) and all(
                np.array_equal(states[call][k].view(np.uint32), want_states[call].view(np.uint32)) for call in range(3))
            if not bits:
                differing += int((pre[c].view(np.uint32) != want.view(np.uint32)).sum())
                worst_pll = max(worst_pll, float(np.abs(pre[c].astype(np.float64) - want).max()) / (level(pairs[c]) / np.sqrt(TOTAL)))
        if ref["anr"][c]:                                                                  # part 3: the filter's arithmetic, bit for bit
            want = lms_of(orc, ref["anr"][c], pre[c])
            assert np.array_equal(audio[c].view(np.uint32), want.view(np.uint32)), (D, kind, c)
        else:
            assert np.array_equal(audio[c].view(np.uint32), pre[c].view(np.uint32)), (D, kind, c)
    print("bank post f32 D %d %s gain %d: pairs %.3e, PLL against the oracle on the device's pairs: %d differing samples, worst %.3e of the pair level"
          % (D, kind, gain, worst_pair, differing, worst_pll))
    assert worst_pair < TOL, worst_pair
    assert worst_pll < TOL, (worst_pll, differing)
    assert np.abs(pre[ref["sync"]]).max() > 1e-3
    for c in chains:
        c.close()


@pytest.mark.parametrize("D, bq", [(1, "rows"), (8, "rows"), (8, "shared")])
def test_cascade_behind_the_pll_and_int16_last(ctx, orc, ref, D, bq):
    """the cascade in CMSIS order (shared or per-channel rows) behind PLL and LMS: arm_biquad_cascade_df1_f32 of the audio in front of it;
    MSDR_CHAIN_OUT_I16 converts last"""
    pre_chain, chain, i16 = make_chain(ctx, ref, D, lms=False), make_chain(ctx, ref, D, bq=bq), make_chain(ctx, ref, D, bq=bq, flags=msdr.CHAIN_OUT_I16)
    pre, _, _, _, _ = run_calls(ctx, pre_chain, ref, D, iq_buf=False)
    audio, _, _, flav, _ = run_calls(ctx, chain, ref, D, iq_buf=False)
    audio16, _, _, _, _ = run_calls(ctx, i16, ref, D, iq_buf=False, dtype=np.int16)
    assert all(f & msdr.FLAVOUR_BANK_POST and f & msdr.FLAVOUR_SEQ_CASCADE and bool(f & msdr.FLAVOUR_CASCADE_PC) == (bq == "rows") for f in flav), flav
    for c in range(CH):
        front = lms_of(orc, ref["anr"][c], pre[c]) if ref["anr"][c] else pre[c]
        want = orc.biquad_df1_zero_state(ref["rows"][c] if bq == "rows" else cascade("lp+notch"), front)
        err = float(np.sqrt(((audio[c].astype(np.float64) - want) ** 2).sum())) / max(level(want), level(pre[c]))
        assert err < TOL, (D, c, err)
        wi = np.clip(np.round(audio[c].astype(np.float64) * 32768.0), -32768, 32767)
        assert np.abs(audio16[c].astype(np.float64) - wi).max() <= 1, (D, c)
    for o in (pre_chain, chain, i16):
        o.close()


def test_end_to_end_on_the_128_grid(ctx, orc, ref):
    """D = 1, steps k 2^25: the bank with the switch on against orc.chain_f32(pll = True) and against the fp32 chain that runs the same channels
    through the auxiliary chain, both within 1e-5 (SYNCAM and plain channels; LMS off: its decisions are discontinuous, the three parts above)"""
    ch, n = 10, 3 * 128
    rng = np.random.default_rng(7201)
    modes = np.array([(AM, SYNCAM)[c % 2] for c in range(ch)], np.int32)
    taps = np.stack([bw_taps(1200.0 + 100.0 * c) for c in range(ch)])
    k = np.array([3, 8, 13, 21, 30, 40, 50, 5, 17, 27], np.uint64)
    t = np.arange(n)
    x = np.stack([np.round(9000 * (1 + 0.3 * np.sin(2 * np.pi * 400 * t / FS)) * np.cos(2 * np.pi * (kk * FS / 128 + 60.0) * t / FS) + rng.normal(0, 60, n)).astype(np.int16) for kk in k])
    ph = ((k[:, None] * np.arange(128, dtype=np.uint64)[None, :]) << np.uint64(25)) & np.uint64(0xFFFFFFFF)
    s, c_ = msdr.nco_q15(ph.astype(np.uint32))
    oi, oq = f32(s.reshape(ch, 128)), f32(c_.reshape(ch, 128))
    bq = cascade("lp")
    bank = msdr.Chain(ctx, msdr.ARITH_F32, ch, taps[0], taps[0], mixer=msdr.MIXER_NCO, modes=modes, biquad_coeffs=bq, flags=msdr.CHAIN_SYNCAM_PLL, osc_i=oi[0], osc_q=oq[0])
    bank.set_bank_post(True)
    bank.set_nco_channels(0, u32(k << np.uint64(25)), u32(np.zeros(ch, np.uint64)))
    bank.set_taps_channels_f32(0, taps)
    dy = ctx.array((ch, n), np.float32)
    bank.process(ctx.to_device(x), dy, n)
    got = dy.download()
    assert bank.post_kernel() == BANK and bank.info()["flavour"] & msdr.FLAVOUR_BANK_POST
    for c in range(ch):
        # the chain the auxiliary route serves: shared taps and tables, one channel each
        aux = msdr.Chain(ctx, msdr.ARITH_F32, 1, taps[c], taps[c], mixer=msdr.MIXER_NCO, modes=modes[c:c + 1], biquad_coeffs=bq, flags=msdr.CHAIN_SYNCAM_PLL, osc_i=oi[c], osc_q=oq[c])
        da = ctx.array((1, n), np.float32)
        aux.process(ctx.to_device(x[c:c + 1]), da, n)
        via_aux = da.download()[0]
        assert aux.post_kernel() == ("post_pll_f32_kernel" if modes[c] == SYNCAM else ""), (c, aux.post_kernel())
        assert not aux.info()["flavour"] & msdr.FLAVOUR_BANK_POST
        aux.close()
        want = orc.chain_f32(x[c], int(modes[c]), taps[c], taps[c], oi[c], oq[c], bq, pll=bool(modes[c] == SYNCAM))
        e_orc = float(np.sqrt(((got[c].astype(np.float64) - want) ** 2).sum())) / level(want)
        e_aux = float(np.sqrt(((got[c].astype(np.float64) - via_aux) ** 2).sum())) / level(via_aux)
        print("bank post f32 end to end ch %d: oracle %.3e, auxiliary chain %.3e" % (c, e_orc, e_aux))
        assert e_orc < TOL and e_aux < TOL, (c, e_orc, e_aux)
    bank.close()


def test_the_meter_is_that_of_a_chain_without_pll_channels(ctx, ref):
    D = 3
    a, b = make_chain(ctx, ref, D), make_chain(ctx, ref, D, lms=False, pll=False, switch=False)
    meters = []
    for chain in (a, b):
        m = ctx.to_device(np.zeros(CH, np.float64))
        chain.set_meter(m)
        run_calls(ctx, chain, ref, D, iq_buf=False, pll=chain is a)
        meters.append(m.download())
        chain.close()
    assert np.array_equal(meters[0].view(np.uint64), meters[1].view(np.uint64)) and meters[0].min() > 0


def test_an_iq_only_call_leaves_the_pll_state_alone_and_the_flavour_follows_the_pass(ctx, ref):
    D = 3
    chain = make_chain(ctx, ref, D)
    _, _, states, flav, names = run_calls(ctx, chain, ref, D, audio_of=lambda call: call != 1)
    assert np.array_equal(states[0].view(np.uint32), states[1].view(np.uint32)) and not np.array_equal(states[1], states[2])
    assert [bool(f & msdr.FLAVOUR_BANK_POST) for f in flav] == [True, False, True], flav
    assert names == [BANK] * 3          # (the PLL kernel of the last AUDIO call)
    # no SYNCAM channel and no LMS channel: no pass, no flavour
    for c in ref["sync"]:
        chain.set_mode(int(c), AM)
    chain.set_anr(None, 0)
    _, _, _, flav, names = run_calls(ctx, chain, ref, D)
    assert not any(f & msdr.FLAVOUR_BANK_POST for f in flav) and names == [""] * 3, (flav, names)
    chain.close()


def test_init_fir_keeps_and_reset_clears_the_pll_and_lms_states(ctx, orc, ref):
    D = 3
    chain, fresh = make_chain(ctx, ref, D), make_chain(ctx, ref, D)
    run_calls(ctx, chain, ref, D, iq_buf=False)
    before = np.stack([chain.pll_state(c) for c in ref["sync"]])
    assert before.any()
    chain.init_fir()
    assert np.array_equal(before.view(np.uint32), np.stack([chain.pll_state(c) for c in ref["sync"]]).view(np.uint32))
    chain.reset()
    assert not np.stack([chain.pll_state(c) for c in ref["sync"]]).any()
    # behind a reset the chain is a fresh one: PLL and LMS start over (the oscillator phases go to 0 on both)
    fresh.reset()
    a, b = run_calls(ctx, chain, ref, D, iq_buf=False)[0], run_calls(ctx, fresh, ref, D, iq_buf=False)[0]
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    chain.close()
    fresh.close()
