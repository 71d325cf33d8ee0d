"""The census of the complex-input chain kernels, fp32 half: one case per fp32 entry of tests/cx_census_cases.py -- every launch geometry
pc_geometry and dec_geometry can hand chain_f32pcn_cx_kernel<CPW> and chain_f32pcnd_cx_kernel<CPW, AL>, every instantiation of their metered,
I/Q and I/Q-plus-meter twins (48 in all; AL = 0 is never selected for fp32).  The recipe, the guard stretches, the reading of chain.info(), the
degenerate form, the history of pairs and part D are those of tests/test_gpu_cx_census.py; the flavour word is asserted too: the parent's bits
(TAPS_PC | NCO_PC, DECIMATED, SHARED_IF, SEGMENTED, and METER / IQ_OUT exactly where set) and COMPLEX_IN exactly on the chains with the mode on.

References and judges are the existing ones, with their present bounds and no new tolerance:
  audio, pairs   tests/cx_cases.py's compose_f32 (freqconv_f32 -> fir_f32_blocks pair -> demod_f32) and compose_f64, per channel at the full rate,
                 outputs at m D + D - 1 of each call; judge_f32 unchanged -- e_go < 1e-5, e_gpu <= 2 e_orc + 1e-6 and e_orc < 2e-6 -- per channel
                 over the calls, the pairs as one row {I, Q} (tests/test_cx_census_cases.py holds every row's e_orc below 2e-6 on the CPU)
  meter          judged of tests/test_gpu_meter_per_channel_f32.py against the composed oracle's sqrt(I^2 + Q^2), per channel and call
and the identities: audio with the tap or the meter on is bit-identical to the plain cx chain, the meter beside the tap is the meter alone,
LSB / USB audio is I -/+ Q of the stored pairs bit for bit, an entry with an input map is bit-identical to the same chain fed the replicated rows
of pairs; dir = 1 over {I, 0} equals the parent's real chain over I as values (a zero may differ in sign)."""
import numpy as np
import pytest

import cx_census_cases as cases
import orclib
import test_gpu_decim_census_f32 as df
import test_gpu_pc_census_f32 as pf
from cx_cases import compose_f32, compose_f64, judge_f32
from gpuhelp import ctx, msdr  # noqa: F401
from test_gpu_cx_census import cached, history_is_what_was_heard, meter_index, part_d, run_cx, with_mode
from test_gpu_decim_census import raw
from test_gpu_iq_per_channel_f32 import ssb_is_the_pairs
from test_gpu_meter_per_channel_f32 import judged as meter_judged

pytestmark = pytest.mark.gpu
F, F64 = np.float32, np.float64
CX = msdr.FLAVOUR_COMPLEX_IN


def refs_f32(orc, e):
    """per channel ((audio, fi, fq) of the fp32 oracle, (audio, fi, fq) in float64) at the full rate"""
    return cached(e, "f32", lambda d, xi, xq, si, sq, c: (compose_f32(orc, xi, xq, si, sq, e["dir"], d["modes"][c], d["ti"][c], d["tq"][c]),
                                                         compose_f64(xi, xq, si, sq, e["dir"], d["modes"][c], d["ti"][c], d["tq"][c])))


def refs_env(orc, e):
    """per channel the composed oracle's sqrt(I^2 + Q^2) at the full rate, whatever the channel's own mode"""
    w = refs_f32(orc, e)
    return cached(e, "env", lambda d, xi, xq, si, sq, c: orc.demod_f32(orclib.AM, w[c][0][1], w[c][0][2]))


def iq_rows(w, idx):
    """(the fp32 oracle's, float64's) pairs [outputs, 2] of one channel"""
    return tuple(np.stack([r[1][idx], r[2][idx]], axis=1) for r in w)


def real_f32(ctx, e, nt=None, inmap=None, decimate=True):
    """the parent entry's chain"""
    if e["kind"] == "pc":
        return pf.make_f32(ctx, e, nt=nt, inmap=inmap)
    chain = df.make_f32(ctx, e, nt)
    if decimate:
        chain.set_decimation(e["D"])
        assert chain.decimation() == e["D"]
    return chain


@pytest.mark.parametrize("name", cases.names(1))
def test_entry(ctx, orc, name):
    e = cases.BY_NAME[name]
    d, ch, idx = cases.data(e), e["channels"], cases.out_index(e)
    meter, iq = "meter" in e["twin"], "iq" in e["twin"]
    want = refs_f32(orc, e)
    base = msdr.FLAVOUR_TAPS_PC | msdr.FLAVOUR_NCO_PC | (msdr.FLAVOUR_DECIMATED if e["kind"] == "dec" else 0)

    def flavour(cx, with_meter, with_iq, with_map):
        def f(info):
            fl = info["flavour"]
            assert fl & (msdr.FLAVOUR_TAPS_PC | msdr.FLAVOUR_OSC_PC | msdr.FLAVOUR_NCO_PC | msdr.FLAVOUR_DECIMATED) == base and bool(fl & CX) == cx, info
            assert bool(fl & msdr.FLAVOUR_METER) == with_meter and bool(fl & msdr.FLAVOUR_IQ_OUT) == with_iq, info
            assert bool(fl & msdr.FLAVOUR_SHARED_IF) == with_map and bool(fl & msdr.FLAVOUR_SEGMENTED) == (e.get("nseg", 1) > 1), info
        return f

    def run(direction, x, with_meter=meter, with_iq=iq, with_map=e["inmap"]):
        """direction None: the parent's real chain"""
        chain = real_f32(ctx, e, inmap=with_map)
        if direction is not None:
            with_mode(chain, direction)
        got = run_cx(ctx, chain, e, x, F, F if with_iq else None, F64 if with_meter else None, flavour(direction is not None, with_meter, with_iq, with_map),
                     replicated=e["inmap"] and not with_map)
        chain.close()
        return got

    audio, pairs, meters, hist = run(e["dir"], d["pairs"])
    for c in range(ch):
        judge_f32("%s ch %d" % (name, c), audio[c], want[c][0][0][idx], want[c][1][0][idx])
        if iq:
            judge_f32("%s ch %d pairs" % (name, c), pairs[c], *iq_rows(want[c], idx))
    if iq:
        ssb_is_the_pairs(audio, pairs, d["modes"])
    if meter:
        env = refs_env(orc, e)
        for c in range(ch):
            e2 = env[c].astype(F64) ** 2
            meter_judged("%s ch %d" % (name, c), meters[:, c], np.array([e2[k].sum() for k in meter_index(e)]))
    # the degenerate form: dir = 1 over {I, 0} is the parent's real chain over I, as values
    r_audio, r_pairs, r_meters, r_hist = run(None, d["x"])
    z_audio, z_pairs, z_meters, z_hist = run(1, d["pairs_q0"])
    assert np.array_equal(z_audio, r_audio) and float(np.abs(r_audio).max()) > 1e-3
    assert (not iq or np.array_equal(z_pairs, r_pairs)) and (not meter or np.array_equal(z_meters, r_meters))
    assert all(zh.shape == rh.shape + (2,) and np.array_equal(zh[:, 0], rh) and not zh[:, 1].any() for zh, rh in zip(z_hist, r_hist))
    history_is_what_was_heard(e, hist, d["pairs"], real_len=r_hist[0].shape[0])
    if e["twin"]:          # the tap and the meter disturb nothing
        plain = run(e["dir"], d["pairs"], False, False)[0]
        assert np.array_equal(raw(audio), raw(plain))
    if meter and iq:       # ... and the tap does not disturb the meter
        alone = run(e["dir"], d["pairs"], True, False)[2]
        assert np.array_equal(raw(meters), raw(alone))
    if e["inmap"]:         # the same chain without the map, fed the replicated rows of pairs
        rep = run(e["dir"], d["pairs"], with_map=False)
        assert np.array_equal(raw(audio), raw(rep[0]))
        history_is_what_was_heard(e, rep[3], d["pairs"])
    if e["refuse"] is not None:
        part_d(ctx, e, lambda nt: pf.make_f32(ctx, e, nt, before=True) if e["kind"] == "pc" else real_f32(ctx, e, nt, decimate=False), F)
