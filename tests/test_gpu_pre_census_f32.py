"""The census of the two-stage decimating chain kernels, fp32 half: one case per fp32 entry of tests/pre_census_cases.py -- every launch geometry
pre_geometry can hand chain_f32pcn2_kernel (45 keys, D1 rotating over them), every (CPW, AL) instantiation of the _full twin with meter, pairs
and gain switched on in turn, the prefilter lengths around a step of 4, the limits of both setters and one call in two time segments per tile.
The recipe, the guard stretches and the reading of chain.info() are those of tests/test_gpu_pre_census.py; the flavour word is asserted too:
PREFILTER | DECIMATED | NCO_PC | TAPS_PC, with METER, IQ_OUT and GAIN exactly where set and SEGMENTED exactly on part F.

References and judges are the existing ones, with their present bounds and no new tolerance:
  audio   cx_cases.judge_f32, unchanged, per channel over the calls: e_go < 1e-5 against tests/prefilter_model.py::model_f32 (the oracle's
          stages composed in fp32), e_gpu <= 2 e_orc + 1e-6 against model_f64, e_orc < 2e-6 (tests/test_pre_census_cases.py shows it on the CPU)
  pairs   1e-5 of the fp32 model's I and Q, as tests/test_gpu_prefilter_per_channel_f32.py holds them
  meter   judged of tests/test_gpu_meter_per_channel_f32.py against the fp32 model's sum of I^2 + Q^2 (ungained), per channel and call
  gain    tests/agc_model.py as tests/test_gpu_agc_per_channel_f32.py applies it: the fp32 sums times the clamped gain, one multiply; the
          device's absmax within 1 of the model's, the records == the rule applied to the device's own absmax, behind every call
and the twins' identities: audio with meter or pairs on is bit-identical to the plain kernel's, LSB / USB audio is I -/+ Q of the stored
pairs bit for bit."""
import numpy as np
import pytest

import agc_model as agc
import pre_census_cases as cases
import prefilter_model as pm
from cx_cases import judge_f32, rel
from gpuhelp import ctx, msdr  # noqa: F401
from test_gpu_decim_census import raw, run_entry
from test_gpu_iq_per_channel_f32 import ssb_is_the_pairs
from test_gpu_meter_per_channel_f32 import judged as meter_judged
from test_gpu_pre_census import osc, part_d, ran, records, switch_on
from test_gpu_prefilter_per_channel_f32 import BASE, nco_chain

pytestmark = pytest.mark.gpu
F, F64 = np.float32, np.float64
_REFS = {}


def refs_f32(orc, e):
    """per channel ((audio, fi, fq) of the fp32 model, (audio, fi, fq) in float64) over the whole stream at the final rate"""
    shape = cases.shape_of(e)
    if shape not in _REFS:
        d = cases.data(e)
        si, sq = osc(e)
        _REFS[shape] = [(pm.model_f32(orc, d["x"][c], si[c], sq[c], d["p"], e["D1"], d["modes"][c], d["ti"][c], d["tq"][c], e["D2"]),
                         pm.model_f64(d["x"][c], si[c], sq[c], d["p"], e["D1"], d["modes"][c], d["ti"][c], d["tq"][c], e["D2"])) for c in range(e["channels"])]
    return _REFS[shape]


def gained_f32(orc, mode, w32, t64, gain):
    """(audio32, (gi, gq), audio64) of outputs under one clamped gain (test_gpu_agc_per_channel_f32.BankF32.expect)"""
    g = agc.clamped(gain)
    gi, gq = (w32[1] * g).astype(F), (w32[2] * g).astype(F)
    hi, hq = t64[1] * float(g), t64[2] * float(g)
    a64 = hi - hq if mode == 2 else hi + hq if mode == 3 else np.sqrt(hi * hi + hq * hq)
    return orc.demod_f32(int(mode), gi, gq), (gi, gq), a64


def make_f32(ctx, e, gain=True):
    d = cases.data(e)
    chain = nco_chain(ctx, e["channels"], d["ti"], d["tq"], d["steps"], d["phases"], modes=d["modes"])
    chain.set_prefilter(e["D1"], d["p"])
    chain.set_decimation(e["D2"])
    assert chain.prefilter() == (e["D1"], e["N1"]) and chain.decimation() == e["D2"]
    if gain:
        switch_on(chain, e)
    return chain


def plain_f32(ctx, e, nt):
    d = cases.data(e)
    assert nt == e["N2"]
    return nco_chain(ctx, e["channels"], d["ti"], d["tq"], d["steps"], d["phases"], modes=d["modes"])


def call_f32(ctx, chain, x):
    D1 = chain.prefilter()[0]
    dy = ctx.array((x.shape[0], x.shape[1] // D1), F)
    chain.process(ctx.to_device(np.ascontiguousarray(x)), dy, x.shape[1])
    return dy.download()


def flavour_of(e, meter, iq, gain):
    def f(info):
        fl = info["flavour"]
        assert fl & BASE == BASE and not fl & (msdr.FLAVOUR_BLOCK | msdr.FLAVOUR_OSC_PC | msdr.FLAVOUR_COMPLEX_IN | msdr.FLAVOUR_SHARED_IF), info
        assert bool(fl & msdr.FLAVOUR_METER) == meter and bool(fl & msdr.FLAVOUR_IQ_OUT) == iq and bool(fl & msdr.FLAVOUR_GAIN) == gain, info
        assert bool(fl & msdr.FLAVOUR_SEGMENTED) == (e["part"] == "F"), info
    return f


@pytest.mark.parametrize("name", cases.names(1))
def test_entry(ctx, orc, name):
    e = cases.BY_NAME[name]
    d = cases.data(e)
    ch, slices = e["channels"], cases.call_slices(e)
    r = refs_f32(orc, e)
    chain = make_f32(ctx, e)
    got_words = []
    audio, pairs, meters = run_entry(ctx, chain, e, F, F if e["iq"] else None, F64 if e["meter"] else None, flavour_of(e, e["meter"], e["iq"], e["gain"]), x=d["x"],
                                     calls=cases.call_outputs(e), ran=ran, read=(0, e["calls"] - 1), after=records(chain, e, got_words), no_audio=not e["out"])
    chain.close()
    rxs = [agc.Rx(f32=True) for _ in range(ch)]
    for c, rx in enumerate(rxs):
        rx.set_gain(d["gains"][c] if e["gain"] else 1.0)
        rx.on = int(e["agc"])
    want32, want64, wantp = np.empty((ch, audio.shape[1]), F), np.empty((ch, audio.shape[1]), F64), np.empty((ch, audio.shape[1], 2), F)
    for k, s in enumerate(slices):          # call by call: an AGC step between two calls changes the gain of the next
        for c, rx in enumerate(rxs):
            (w32, t64), mode = r[c], int(d["modes"][c])
            if e["gain"]:
                want32[c, s], (gi, gq), want64[c, s] = gained_f32(orc, mode, [v[s] for v in w32], [v[s] for v in t64], rx.val)
                dev, model_absmax = int(got_words[k][c][3]), rx.absmax_of(gi, gq)
                print("pre census %s call %d ch %d absmax device %d model %d" % (name, k, c, dev, model_absmax))
                assert abs(dev - model_absmax) <= 1, (k, c, dev, model_absmax)
                rx.after_call(dev)          # the rule on the device's own absmax
                assert np.array_equal(got_words[k][c], rx.words()), (k, c, got_words[k][c].tolist(), rx.words().tolist())
            else:
                want32[c, s], want64[c, s], (gi, gq) = w32[0][s], t64[0][s], (w32[1][s], w32[2][s])
            wantp[c, s, 0], wantp[c, s, 1] = gi, gq
    for c in range(ch):
        if e["out"]:
            judge_f32("%s ch %d" % (name, c), audio[c], want32[c], want64[c])
        if e["iq"]:
            for j, stream in enumerate(("fi", "fq")):
                err = rel(pairs[c, :, j], wantp[c, :, j])
                print("pre census %s ch %d %s %.3e" % (name, c, stream, err))
                assert err < 1e-5, (c, stream, err)
        if e["meter"]:          # the meter keeps the ungained pair
            w32 = r[c][0]
            meter_judged("%s ch %d" % (name, c), meters[:, c], np.array([(w32[1][s].astype(F64) ** 2 + w32[2][s].astype(F64) ** 2).sum() for s in slices]))
    if e["iq"] and e["out"]:
        ssb_is_the_pairs(audio, pairs, d["modes"])
    if e["agc"]:
        assert all(rx.steps == e["calls"] for rx in rxs)
    if e["full"] and e["out"] and not e["gain"]:          # meter and pairs disturb nothing: the plain kernel gives the same bits
        off = make_f32(ctx, e)
        plain, _, _ = run_entry(ctx, off, e, F, None, None, flavour_of(e, False, False, False), x=d["x"], calls=cases.call_outputs(e), ran=ran, read=(0, e["calls"] - 1))
        off.close()
        assert np.array_equal(raw(audio), raw(plain))
    if e["part"] == "D":
        long_row = np.concatenate([np.full(e["refuse"] - e["N1"], 1e-4, F), d["p"]]) if e["limit"] == "taps" else None
        part_d(ctx, e, lambda nt: plain_f32(ctx, e, nt), lambda chain, x: call_f32(ctx, chain, x), long_row)
