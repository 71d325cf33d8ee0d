"""Shared IF input: msdr_chain_set_input_rows -- one antenna stream (or a few) feeds a bank of receivers.  d_if is [n_inputs][n] and receiver c
hears row input_row[c]; it must produce, bit for bit, what it would produce if d_if[c] held a copy of that row, with every state kept and
the FIR history per channel.

Shapes: 9 channels (not a multiple of the 4 channels a wave serves at block cadence: the last wave is partly idle) on 3 rows, the map
[2,0,0,1,2,2,1,0,2] (non-monotone, with repeats: one wave's four channels meet equal and different rows); 102 taps and 8 (Q15) / 5 (fp32);
osc_len 128.  The [n_inputs][n] input lies at the start of a device buffer of the replicated size [channels][n] whose rest holds a non-zero
sentinel: a kernel that ignored the map would read defined memory and fail the comparison.

References.  Q15: orclib.Oracle.chain_q15 per receiver on its mapped row, np.array_equal.  fp32: a twin chain with the identity input that
is handed host-gathered rows -- the same kernel doing the same operations, so bit-identical audio and cascade state -- and, for one case,
float64 through f32judge under the per-channel tests' criterion (e_go < 1e-5, float64 clause at level 1)."""
import ctypes as C

import numpy as np
import pytest
from scipy.signal import lfilter

import orclib
from f32judge import fp32_noise, judge
from f32pc_cases import bw_taps as bw_taps_f32, cascade, hilbert_pair
from gpuhelp import ctx, msdr  # noqa: F401

pytestmark = pytest.mark.gpu
B = 128
L = 128
CH, NI = 9, 3
MAP = np.array([2, 0, 0, 1, 2, 2, 1, 0, 2], np.uint32)
SENTINEL = 0x5A5A
CORR = orclib.AUDIO_SAMPLE_RATE_EXACT / 24000.0
AM, LSB, USB, CW, SYNCAM = orclib.AM, orclib.LSB, orclib.USB, orclib.CW, orclib.SYNCAM
MODES = np.array([(AM, LSB, USB, CW)[c % 4] for c in range(CH)], np.int32)


def bw_taps(bw, n):
    return msdr.calc_fir_coeffs(n, float(bw), 70.0, 0, 0.0, 24000.0)[:n].copy()


def q15_rows(ch, seed=0):
    k = (1 + seed + 3 * np.arange(ch)) % L
    ph = 0.37 * (1 + seed) + 0.61 * np.arange(ch)
    a = 2 * np.pi * k[:, None] * np.arange(L)[None, :] / L + ph[:, None]
    return np.round(32767 * np.sin(a)).astype(np.int16), np.round(32767 * np.cos(a)).astype(np.int16)


def f32_rows(ch, seed=0):
    oi, oq = q15_rows(ch, seed)
    return (oi / 32768.0).astype(np.float32), (oq / 32768.0).astype(np.float32)


def shared(ctx, xin, ch):
    """xin [n_inputs, n] at the start of a device buffer of the replicated size [ch, n]; the rest is the sentinel"""
    full = np.full((ch, xin.shape[1]), SENTINEL, np.int16)
    full.reshape(-1)[:xin.size] = xin.reshape(-1)
    return ctx.to_device(full)


def run(ctx, chain, xin, ch, steps, dtype=np.int16):
    """the calls of `steps` samples each, one after the other, over xin [rows, sum(steps)]; rows < ch: the shared buffer"""
    got = np.empty((ch, xin.shape[1]), dtype)
    o = 0
    for m in steps:
        part = np.ascontiguousarray(xin[:, o:o + m])
        dx, dy = shared(ctx, part, ch) if part.shape[0] < ch else ctx.to_device(part), ctx.array((ch, m), dtype)
        chain.process(dx, dy, m)
        got[:, o:o + m] = dy.download()
        o += m
    assert o == xin.shape[1]
    return got


def q15_oracle(orc, x, mode, ci, cq, osc=None, nodes=(), want_iq=False):
    """one receiver from zero state over a stream of any length: zeros are appended up to whole 128-sample blocks (the chain is causal) and cut off again"""
    n = x.size
    xp = np.zeros(-(-n // B) * B, np.int16)
    xp[:n] = x
    st, out = {}, []
    for b in range(xp.size // B):
        sl = slice(b * B, (b + 1) * B)
        kw = dict(mixer=1, osc_i=osc[0][(sl.start + np.arange(B)) % L], osc_q=osc[1][(sl.start + np.arange(B)) % L]) if osc is not None else {}
        r = orc.chain_q15(xp[sl], int(mode), ci, cq, state=st, want_iq=want_iq, **kw)
        if not want_iq:
            for nd in nodes:
                r = orc.biquad_teensy_update(nd, r)
        out.append(r)
    if want_iq:
        return [np.concatenate(p)[:n] for p in zip(*out)]
    return np.concatenate(out)[:n]


def history_is_the_mapped_row(chain, xin, rows):
    for c, r in enumerate(rows):
        h = chain.fir_history(c)
        tail = np.concatenate([np.zeros(max(0, h.size - xin.shape[1]), np.int16), xin[r, -h.size:]])
        assert np.array_equal(h, tail), c


STEPS = [B] * 6 + [1000]            # six ticks (4 channels per wave) and one long call (1 per wave, time segments)


# ------------------------------------------------------------------------------------------------ 1 + 2. Q15: the oracle, the replicated chain
@pytest.mark.parametrize("case", ["fs4_taps", "nco_osc", "nodes"])
def test_q15_against_the_oracle_and_the_replicated_chain(ctx, orc, case):
    rng = np.random.default_rng({"fs4_taps": 1, "nco_osc": 2, "nodes": 3}[case])
    nt = 8 if case == "nco_osc" else 102
    n = sum(STEPS)
    x = rng.integers(-30000, 30001, (NI, n)).astype(np.int16)
    taps = np.stack([bw_taps(500.0 + 350.0 * c, nt) for c in range(CH)])
    oi, oq = q15_rows(CH)
    lp = msdr.biquad_design(msdr.BQ_LOWPASS, np.float32(5400.0 * CORR), 0.54)
    notch = [msdr.biquad_design(msdr.BQ_NOTCH, np.float32((3000.0 + 2.6 * c) * CORR), 15.0) for c in range(CH)]

    def make():
        if case == "fs4_taps":
            ch = msdr.Chain(ctx, msdr.ARITH_Q15, CH, taps[0], taps[0], modes=MODES)
            ch.set_taps_channels(0, taps)
        elif case == "nco_osc":
            ch = msdr.Chain(ctx, msdr.ARITH_Q15, CH, taps[0], taps[0], mixer=msdr.MIXER_NCO, modes=MODES, osc_i=oi[0], osc_q=oq[0])
            ch.set_osc_channels(0, oi, oq)
        else:
            ch = msdr.Chain(ctx, msdr.ARITH_Q15, CH, taps[0], taps[0], modes=MODES, biquad_nodes=[[lp], [notch[0]]])
            ch.set_node_coefficients_channels(1, 0, 0, np.stack(notch))
        return ch

    chain, twin = make(), make()
    chain.set_input_rows(MAP)
    if case == "nodes":              # (the twin enters the per-channel kernel family by the door it has: rows that repeat the shared set)
        twin.set_taps_channels(0, np.tile(taps[0], (CH, 1)))
    got = run(ctx, chain, x, CH, STEPS)
    info = chain.info()
    assert info["kernel"].startswith("chain_q15pco_kernel" if case == "nco_osc" else "chain_q15pc_kernel"), info
    assert info["time_segments"] > 1 or info["tile"] == 512, info
    for c in range(CH):
        ci = taps[c] if case == "fs4_taps" else taps[0]
        nodes = ()
        if case == "nodes":
            nodes = [orc.biquad_teensy_new([lp]), orc.biquad_teensy_new([notch[0]])]
            orc.lib.orc_biquad_teensy_set_coefficients(C.byref(nodes[1]), C.c_uint32(0), orclib._ptr(np.ascontiguousarray(notch[c], np.int32)))
        want = q15_oracle(orc, x[MAP[c]], MODES[c], ci, ci, osc=(oi[c], oq[c]) if case == "nco_osc" else None, nodes=nodes)
        assert np.array_equal(got[c], want), (case, c)
    history_is_the_mapped_row(chain, x, MAP)
    # 2. the replicated chain: identity input, host-gathered rows
    assert np.array_equal(got, run(ctx, twin, x[MAP], CH, STEPS))
    assert twin.info()["kernel"] == info["kernel"]
    chain.close()
    twin.close()


# ------------------------------------------------------------------------------------------------ 3. fp32: bit-identical to the replicated chain
def f32_bank(nt):
    ssb, cw = hilbert_pair(nt), hilbert_pair(nt, 700.0, 300.0)
    ti = np.stack([bw_taps_f32(500.0 + 350.0 * c, nt) if MODES[c] == AM else (cw if MODES[c] == CW else ssb)[0] for c in range(CH)])
    tq = np.stack([ti[c] if MODES[c] == AM else (cw if MODES[c] == CW else ssb)[1] for c in range(CH)])
    return ti, tq


def f32_pair(ctx, kind, nt, flags=0, bq_rows=None, bq=None):
    """(chain, twin) in the same kernel family: kind fs4 / nco (chain_f32pc_kernel) / pco (chain_f32pco_kernel)"""
    ti, tq = f32_bank(nt)
    oi, oq = f32_rows(CH)
    out = []
    for _ in range(2):
        kw = dict(mixer=msdr.MIXER_NCO, osc_i=oi[0], osc_q=oq[0]) if kind != "fs4" else {}
        ch = msdr.Chain(ctx, msdr.ARITH_F32, CH, ti[0], tq[0], modes=MODES, flags=flags,
                        biquad_coeffs=bq if bq is not None else (bq_rows[0] if bq_rows is not None else None), **kw)
        ch.set_taps_channels_f32(0, ti, tq)
        if kind == "pco":
            ch.set_osc_channels(0, oi, oq)
        if bq_rows is not None:
            ch.set_biquad_coeffs_channels(0, bq_rows)
        out.append(ch)
    return out[0], out[1], (ti, tq, oi, oq)


def cascade_rows():
    """two stages per receiver: the low-pass and the notch with another numerator gain each (poles untouched)"""
    base = cascade("lp+notch")
    r = np.stack([base.copy() for _ in range(CH)])
    for c in range(CH):
        r[c, :, :3] *= np.float32(1.0 - 0.03 * c)
    return r


@pytest.mark.parametrize("i16", [0, 1])
@pytest.mark.parametrize("kind,nt", [("fs4", 102), ("nco", 5), ("pco", 102)])
def test_f32_bit_identical_to_the_replicated_chain(ctx, kind, nt, i16):
    rng = np.random.default_rng(30 + i16)
    dt = np.int16 if i16 else np.float32
    chain, twin, _ = f32_pair(ctx, kind, nt, flags=msdr.CHAIN_OUT_I16 if i16 else 0, bq_rows=cascade_rows())
    chain.set_input_rows(MAP)
    main = "chain_f32pco_kernel" if kind == "pco" else "chain_f32pc_kernel"
    # block kernel off: three ticks and one long call; then on: ticks of 128 and of 32 (the same chains: every state moves over)
    plan = [(False, [B] * 3 + [1000], main), (True, [B] * 2, "chain_f32pcb_kernel"), (True, [32] * 4, "chain_f32pcb_kernel"), (False, [B], main)]
    for on, steps, name in plan:
        for o in (chain, twin):
            o.set_block_kernel(on)
        x = rng.integers(-20000, 20001, (NI, sum(steps))).astype(np.int16)
        got, want = run(ctx, chain, x, CH, steps, dt), run(ctx, twin, x[MAP], CH, steps, dt)
        assert got.tobytes() == want.tobytes(), (kind, i16, on, steps[0], float(np.abs(got.astype(np.float64) - want).max()))
        a, b = chain.info(), twin.info()
        assert a["kernel"].startswith(name) and a["kernel"] == b["kernel"], (a, b)
        assert a["flavour"] == b["flavour"] | msdr.FLAVOUR_SHARED_IF and not b["flavour"] & msdr.FLAVOUR_SHARED_IF, (a, b)
        assert {k: v for k, v in a.items() if k != "flavour"} == {k: v for k, v in b.items() if k != "flavour"}
        for c in range(CH):
            assert chain.cmsis_state(c).tobytes() == twin.cmsis_state(c).tobytes(), c
        if sum(steps) >= 1000:
            history_is_the_mapped_row(chain, x, MAP)
    chain.set_input_rows(None)          # back to the identity: the bit goes, the states stay
    x = rng.integers(-20000, 20001, (CH, B)).astype(np.int16)
    assert run(ctx, chain, x, CH, [B], dt).tobytes() == run(ctx, twin, x, CH, [B], dt).tobytes()
    assert chain.info() == twin.info() and not chain.info()["flavour"] & msdr.FLAVOUR_SHARED_IF
    chain.close()
    twin.close()


def test_f32_against_float64(ctx, orc):
    """chain_f32pco_kernel + the shared two-stage cascade, six ticks, every receiver judged as tests/test_gpu_osc_per_channel_f32.py judges"""
    rng = np.random.default_rng(33)
    bq = cascade("lp+notch")
    chain, twin, (ti, tq, oi, oq) = f32_pair(ctx, "pco", 102, bq=bq)
    twin.close()
    chain.set_input_rows(MAP, n_inputs=NI)
    n = 6 * B
    x = rng.integers(-20000, 20001, (NI, n)).astype(np.int16)
    got = run(ctx, chain, x, CH, [B] * 6, np.float32)
    assert chain.info()["flavour"] & msdr.FLAVOUR_SHARED_IF
    for c in range(CH):
        xr = x[MAP[c]]
        si, sq = oi[c][np.arange(n) % L], oq[c][np.arange(n) % L]
        want = orc.chain_f32(xr, int(MODES[c]), ti[c], tq[c], si, sq, bq)
        pre = orc.chain_f32(xr, int(MODES[c]), ti[c], tq[c], si, sq, None)
        xf = xr.astype(np.float64) / 32768.0
        ai = lfilter(ti[c].astype(np.float64)[::-1], [1.0], xf * sq.astype(np.float64))
        aq = lfilter(tq[c].astype(np.float64)[::-1], [1.0], xf * si.astype(np.float64))
        d = ai - aq if MODES[c] == LSB else ai + aq if MODES[c] == USB else np.sqrt(ai * ai + aq * aq)
        for s in np.asarray(bq, np.float64):
            d = lfilter(s[:3], [1.0, -s[3], -s[4]], d)
        e_go, e_gpu, e_orc, bound = judge(got[c], xr, dict(bq=bq), refs=(want, d, pre))
        b1 = 2 * e_orc + fp32_noise(bq) + 1e-6
        print("ch %d e_go %.3e e_gpu %.3e e_orc %.3e bound %.3e" % (c, e_go, e_gpu, e_orc, b1))
        assert e_go < 1e-5, (c, "first clause", e_go)
        assert e_gpu <= min(bound, b1), (c, "float64 clause", e_gpu, b1)
    chain.close()


# ------------------------------------------------------------------------------------------------ 4. rows that start at different misalignments
def test_misaligned_rows(ctx, orc):
    """n = 130: the row stride is 260 bytes, so the three rows start 0, 4 and 8 bytes past a 16-byte boundary (the unfused launches)"""
    rng = np.random.default_rng(4)
    n, calls = 130, 3
    x = rng.integers(-30000, 30001, (NI, n * calls)).astype(np.int16)
    taps = np.stack([bw_taps(500.0 + 350.0 * c, 102) for c in range(CH)])
    oi, oq = q15_rows(CH)
    q, qt = (msdr.Chain(ctx, msdr.ARITH_Q15, CH, taps[0], taps[0], mixer=msdr.MIXER_NCO, modes=MODES, osc_i=oi[0], osc_q=oq[0]) for _ in range(2))
    for o in (q, qt):
        o.set_taps_channels(0, taps)
        o.set_osc_channels(0, oi, oq)
    q.set_input_rows(MAP)
    got = run(ctx, q, x, CH, [n] * calls)
    for c in range(CH):
        assert np.array_equal(got[c], q15_oracle(orc, x[MAP[c]], MODES[c], taps[c], taps[c], osc=(oi[c], oq[c]))), c
    assert np.array_equal(got, run(ctx, qt, x[MAP], CH, [n] * calls))
    history_is_the_mapped_row(q, x, MAP)
    q.close()
    qt.close()
    for kind in ("fs4", "pco"):
        f, ft, _ = f32_pair(ctx, kind, 102, bq_rows=cascade_rows())
        f.set_block_kernel(True)          # (n = 130 is no block-cadence length: the unfused launches run all the same)
        ft.set_block_kernel(True)
        f.set_input_rows(MAP)
        a, b = run(ctx, f, x, CH, [n] * calls, np.float32), run(ctx, ft, x[MAP], CH, [n] * calls, np.float32)
        assert a.tobytes() == b.tobytes(), kind
        assert not f.info()["kernel"].startswith("chain_f32pcb_kernel")
        history_is_the_mapped_row(f, x, MAP)
        f.close()
        ft.close()


# ------------------------------------------------------------------------------------------------ 5. live remap and the return to identity
@pytest.mark.parametrize("arith", ["q15", "f32", "f32_block"])
def test_live_remap_and_return(ctx, arith):
    """the map changes after tick 2 (an antenna switch: every receiver carries on over its own history) and goes after tick 4"""
    rng = np.random.default_rng(5)
    map2 = np.array([0, 0, 1, 2, 1, 0, 2, 2, 1], np.uint32)
    dt = np.int16 if arith == "q15" else np.float32
    if arith == "q15":
        taps = np.stack([bw_taps(500.0 + 350.0 * c, 102) for c in range(CH)])
        oi, oq = q15_rows(CH)
        chain, twin = (msdr.Chain(ctx, msdr.ARITH_Q15, CH, taps[0], taps[0], mixer=msdr.MIXER_NCO, modes=MODES, osc_i=oi[0], osc_q=oq[0]) for _ in range(2))
        for o in (chain, twin):
            o.set_osc_channels(0, oi, oq)
    else:
        chain, twin, _ = f32_pair(ctx, "pco", 102, bq_rows=cascade_rows())
        for o in (chain, twin):
            o.set_block_kernel(arith == "f32_block")
    chain.set_input_rows(MAP)
    for k in range(6):
        if k == 3:
            chain.set_input_rows(map2, n_inputs=NI)
        if k == 5:
            chain.set_input_rows(None)
        rows = MAP if k < 3 else map2 if k < 5 else np.arange(CH)
        x = rng.integers(-25000, 25001, (NI if k < 5 else CH, B)).astype(np.int16)
        a, b = run(ctx, chain, x, CH, [B], dt), run(ctx, twin, x[rows], CH, [B], dt)
        assert a.tobytes() == b.tobytes(), (arith, k)
        for c in range(CH):
            assert np.array_equal(chain.fir_history(c), twin.fir_history(c)), (k, c)
    chain.close()
    twin.close()


# ------------------------------------------------------------------------------------------------ 6. one stream, five receivers
def test_one_stream_five_receivers(ctx, orc):
    rng = np.random.default_rng(6)
    ch, nt = 5, 102
    taps = bw_taps(2400.0, nt)
    oi, oq = q15_rows(ch, seed=4)
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, ch, taps, taps, mixer=msdr.MIXER_NCO, mode=AM, osc_i=oi[0], osc_q=oq[0])
    chain.set_osc_channels(0, oi, oq)
    chain.set_input_rows(np.zeros(ch, np.int64))
    x = rng.integers(-30000, 30001, (1, 4 * B)).astype(np.int16)
    got = run(ctx, chain, x, ch, [B] * 4)
    for c in range(ch):
        assert np.array_equal(got[c], q15_oracle(orc, x[0], AM, taps, taps, osc=(oi[c], oq[c]))), c
    assert len({got[c].tobytes() for c in range(ch)}) == ch
    chain.close()


# ------------------------------------------------------------------------------------------------ 7. refusals leave the chain untouched
def test_refusals_leave_the_chain_untouched(ctx):
    rng = np.random.default_rng(7)
    lib = ctx.lib
    ERR = msdr.STATUS_ARGUMENT_ERROR

    def call(chain, ni, rows):
        return lib.msdr_chain_set_input_rows(chain.h if chain is not None else None, C.c_uint32(ni), None if rows is None else rows.ctypes.data_as(C.c_void_p))

    def same_next_tick(a, b, dt, rows=None):
        x = rng.integers(-20000, 20001, (CH if rows is None else NI, B)).astype(np.int16)
        ga, gb = run(ctx, a, x, CH, [B], dt), run(ctx, b, x if rows is None else x[rows], CH, [B], dt)
        assert ga.tobytes() == gb.tobytes()

    taps = bw_taps(2400.0, 102)
    q, qt = (msdr.Chain(ctx, msdr.ARITH_Q15, CH, taps, taps, modes=MODES) for _ in range(2))
    assert call(None, NI, MAP) == ERR and call(None, 0, None) == ERR
    bad = MAP.copy()
    bad[8] = NI
    assert call(q, NI, bad) == ERR                                    # an entry >= n_inputs
    assert call(q, NI, None) == ERR                                   # NULL array with n_inputs > 0
    with pytest.raises(ValueError):
        q.set_input_rows(MAP, n_inputs=2)
    same_next_tick(q, qt, np.int16)
    assert q.info() == qt.info() and "pc_kernel" not in q.info()["kernel"]          # not even the change of kernel
    # ... and a chain that has a map keeps it
    q.set_input_rows(MAP)
    assert call(q, NI, bad) == ERR and call(q, NI, None) == ERR
    qt.set_taps_channels(0, np.tile(taps, (CH, 1)))
    same_next_tick(q, qt, np.int16, MAP)
    q.close()
    qt.close()

    ti, tq = f32_bank(102)
    pm = np.array([AM, SYNCAM, AM, LSB, SYNCAM, AM, USB, AM, AM], np.int32)
    p, pt = (msdr.Chain(ctx, msdr.ARITH_F32, CH, ti[0], tq[0], modes=pm, flags=msdr.CHAIN_SYNCAM_PLL) for _ in range(2))
    assert call(p, NI, MAP) == ERR and call(p, 0, None) == ERR         # fp32 + MSDR_CHAIN_SYNCAM_PLL
    same_next_tick(p, pt, np.float32)
    assert p.info() == pt.info()
    p.close()
    pt.close()
    anr = np.array([0, 0, 1, 0, 0, 0, 0, 0, 0], np.int32)
    a, at = (msdr.Chain(ctx, msdr.ARITH_F32, CH, ti[0], tq[0], modes=MODES) for _ in range(2))
    for o in (a, at):
        o.set_anr(anr)
    assert call(a, NI, MAP) == ERR                                     # an LMS channel of an fp32 chain is on
    same_next_tick(a, at, np.float32)
    assert a.info() == at.info()
    for o in (a, at):
        o.set_anr(None, 0)
    a.set_input_rows(MAP)                                              # ... off: accepted, and then set_anr with a channel on is refused
    at.set_taps_channels_f32(0, np.tile(ti[0], (CH, 1)), np.tile(tq[0], (CH, 1)))          # (the twin's door into the same kernel family: the shared set in every row)
    with pytest.raises(msdr.MsdrError) as e:
        a.set_anr(anr)
    assert e.value.status == ERR
    a.set_anr(None, 0)                                                 # (nothing on: fine)
    same_next_tick(a, at, np.float32, MAP)
    a.close()
    at.close()


# ------------------------------------------------------------------------------------------------ 8. Q15: PLL and LMS channels behind the kernel
def test_q15_syncam_pll_and_an_lms_channel_with_a_map(ctx, orc):
    rng = np.random.default_rng(8)
    n = 6 * B
    t = np.arange(n)
    x = np.stack([(9000 * (1 + 0.5 * np.sin(2 * np.pi * 400 * t / 24000)) * np.cos(2 * np.pi * 6000 * t / 24000 + r)
                   + 1500 * np.cos(2 * np.pi * 7000 * t / 24000) + rng.integers(-100, 101, n)).astype(np.int16) for r in range(NI)])
    taps = np.stack([bw_taps(2000.0 + 300.0 * c, 102) for c in range(CH)])
    modes = np.array([AM, SYNCAM, AM, AM, SYNCAM, AM, AM, SYNCAM, AM], np.int32)
    anr_on = np.array([0, 0, 1, 0, 0, 0, 0, 0, 0], np.int32)
    a = 2 * np.pi * (30 + np.arange(CH) % 5)[:, None] * np.arange(L)[None, :] / L + 0.3 * np.arange(CH)[:, None]
    oi, oq = np.round(32767 * np.sin(a)).astype(np.int16), np.round(32767 * np.cos(a)).astype(np.int16)
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, CH, taps[0], taps[0], mixer=msdr.MIXER_NCO, modes=modes, osc_i=oi[0], osc_q=oq[0], flags=msdr.CHAIN_SYNCAM_PLL)
    chain.set_anr(anr_on)
    chain.set_input_rows(MAP)
    chain.set_osc_channels(0, oi, oq)
    chain.set_taps_channels(0, taps)
    got = run(ctx, chain, x, CH, [B] * 6)
    assert chain.info()["kernel"].startswith("chain_q15pco_kernel")
    for c in range(CH):
        audio, i_f, q_f = q15_oracle(orc, x[MAP[c]], AM, taps[c], taps[c], osc=(oi[c], oq[c]), want_iq=True)
        if modes[c] == SYNCAM:
            audio = orc.syncam_q15(orc.syncam_new(), i_f, q_f)
        audio = orc.anr_q15(orc.anr_new(), anr_on[c], audio)
        assert np.array_equal(got[c], audio), c
    chain.close()


# ------------------------------------------------------------------------------------------------ 9. HIP graphs
@pytest.mark.parametrize("arith", ["q15", "f32"])
def test_graphs(ctx, arith):
    rng = np.random.default_rng(9)
    T = 2
    dt = np.int16 if arith == "q15" else np.float32
    if arith == "q15":
        taps = np.stack([bw_taps(500.0 + 350.0 * c, 102) for c in range(CH)])
        chain, twin = (msdr.Chain(ctx, msdr.ARITH_Q15, CH, taps[0], taps[0], modes=MODES) for _ in range(2))
        for o in (chain, twin):
            o.set_taps_channels(0, taps)
    else:
        chain, twin, _ = f32_pair(ctx, "fs4", 102, bq_rows=cascade_rows())
        for o in (chain, twin):
            o.set_block_kernel(True)
    dxs, dys = [ctx.array((CH, B), np.int16) for _ in range(T)], [ctx.array((CH, B), dt) for _ in range(T)]

    def replay(g, rows, tag):
        x = rng.integers(-20000, 20001, (CH if rows is None else NI, T * B)).astype(np.int16)
        for j in range(T):
            full = np.full((CH, B), SENTINEL, np.int16)
            full.reshape(-1)[:x.shape[0] * B] = x[:, j * B:(j + 1) * B].reshape(-1)
            dxs[j].upload(full)
        g.launch()
        got = np.concatenate([dys[j].download() for j in range(T)], axis=1)
        assert got.tobytes() == run(ctx, twin, x if rows is None else x[rows], CH, [B] * T, dt).tobytes(), tag

    def refused(g):
        with pytest.raises(msdr.MsdrError) as e:
            g.launch()
        assert e.value.status == msdr.STATUS_ARGUMENT_ERROR
        g.close()

    g = chain.graph(dxs, dys, B)
    replay(g, None, "before")
    chain.set_input_rows(MAP)
    refused(g)                                                         # made before the call
    g = chain.graph(dxs, dys, B)
    replay(g, MAP, "replay 1")
    replay(g, MAP, "replay 2")
    x = rng.integers(-20000, 20001, (NI, T * B)).astype(np.int16)       # direct calls between replays
    assert run(ctx, chain, x, CH, [B] * T, dt).tobytes() == run(ctx, twin, x[MAP], CH, [B] * T, dt).tobytes()
    replay(g, MAP, "replay 3")
    chain.set_input_rows(MAP)                                          # any later call, the same map included
    refused(g)
    g = chain.graph(dxs, dys, B)
    replay(g, MAP, "replay 4")
    chain.set_input_rows(None)                                         # the return to the identity
    refused(g)
    g = chain.graph(dxs, dys, B)
    replay(g, None, "identity again")
    g.close()
    chain.close()
    twin.close()
