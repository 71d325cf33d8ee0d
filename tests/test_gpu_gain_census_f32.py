"""The census of the gain twins, fp32 half: one case per fp32 entry of tests/gain_census_cases.py -- every launch geometry pc_geometry and
dec_geometry can hand chain_f32pcn[_cx]_gain_kernel<CPW> and chain_f32pcnd[_cx]_gain_kernel<CPW, AL> (24 instantiations; AL = 0 is never
selected for fp32).  The recipe, the guard stretches, the reading of chain.info() and the records behind every call are those of
tests/test_gpu_gain_census.py; the flavour word is asserted too: TAPS_PC | NCO_PC (and DECIMATED behind a factor) with GAIN set, METER / IQ_OUT
exactly where set, COMPLEX_IN exactly on the complex entries, SHARED_IF under an input map and SEGMENTED where the rule gives segments.

The model is tests/test_gpu_agc_per_channel_f32.py::BankF32 (the fp32 oracle's FIR sums of cx_cases.compose_f32 times the receiver's clamped
gain, one fp32 multiply, then orc.demod_f32; the same chain in float64), call by call under the gains the records hold.  No new tolerance:
  audio    per receiver over the three calls, the two clauses as test_gpu_agc_per_channel_f32.judged applies them: e_go < 1e-5 against the fp32
           model and e_gpu <= 2 e_orc + 1e-6 against float64 (tests/test_gain_census_cases.py holds e_orc < 2e-6 on every judged receiver, on
           the CPU: cx_cases.judge_f32's third clause); a receiver with a zero gain is held to exact zeros, audio and pairs
  pairs    the row {I, Q} of a receiver over the three calls to 1e-5 of the fp32 model's gained pair
  meter    judged of tests/test_gpu_meter_per_channel_f32.py against the UNGAINED sum, per receiver and call
  absmax   the device's within 1 of the model's; records == the rule applied to the device's own absmax, behind every call
  identity LSB / USB audio is I -/+ Q of the stored pairs bit for bit, wherever audio and pairs both exist
Every figure is printed."""
import numpy as np
import pytest

import agc_model as M
import gain_census_cases as cases
from cx_cases import rel
from gpuhelp import ctx, msdr  # noqa: F401
from test_gpu_agc_per_channel_f32 import BankF32
from test_gpu_decim_per_channel_f32 import nco_chain
from test_gpu_gain_census import fresh, run_gain, spans, streams, switch_on
from test_gpu_iq_per_channel_f32 import ssb_is_the_pairs
from test_gpu_meter_per_channel_f32 import judged as meter_judged

pytestmark = pytest.mark.gpu
F, F64 = np.float32, np.float64
_BANKS = {}


def bank_f32(orc, e):
    key = (cases.shape_of(e), e["cx"], e["dir"])
    if key not in _BANKS:
        d = cases.data(e)
        xi, xq, si, sq = streams(e)
        _BANKS[key] = BankF32(orc, xi, xq, si, sq, d["modes"], d["ti"], d["tq"], direction=e["dir"])
    return fresh(_BANKS[key], e, f32=True)


def model_f32(orc, e, device_words=None, tag=""):
    """the entry by the model, call by call: audio32, audio64 [ch, outputs], pairs32 [ch, outputs, 2], meters [calls, ch] (ungained), the
    receivers' records behind every call and of the last call per receiver `true` and `longer` (gain_census_cases' part D).  device_words:
    the records a chain returned behind every call -- the device's absmax is then held to within 1 of the model's and the rule steps on the
    device's own (without: on the model's)"""
    bank = bank_f32(orc, e)
    ch, D = e["channels"], cases.factor(e)
    total = sum(cases.calls(e))
    a32, a64, p32 = np.empty((ch, total), F), np.empty((ch, total), F64), np.empty((ch, total, 2), F)
    meters, words, longer = [], [[rx.words() for rx in bank.rx]], []
    for k, ((lo, hi), s) in enumerate(zip(spans(e), cases.call_slices(e))):
        idx = M.out_index(lo, hi, D)
        row = []
        for c, rx in enumerate(bank.rx):
            if k == 2:
                gi, gq = bank.expect(c, M.out_index(lo, hi + cases.pad(e), D))[1]
                longer.append(rx.absmax_of(gi, gq))
            a32[c, s], (gi, gq), a64[c, s], energy = bank.expect(c, idx)
            p32[c, s, 0], p32[c, s, 1] = gi, gq
            row.append(energy)
            absmax = rx.absmax_of(gi, gq)
            if device_words is not None:
                dev = int(device_words[k + 1][c][3])
                print("gain census %s call %d ch %d absmax device %d model %d" % (tag, k, c, dev, absmax))
                assert abs(dev - absmax) <= 1, (tag, k, c, dev, absmax)
                absmax = dev
            rx.after_call(absmax)
        meters.append(row)
        words.append([rx.words() for rx in bank.rx])
    return dict(audio32=a32, audio64=a64, pairs=p32, meters=np.array(meters), words=words, true=[rx.absmax for rx in bank.rx], longer=longer, bank=bank)


def make_f32(ctx, e):
    d, ch = cases.data(e), e["channels"]
    chain = nco_chain(ctx, ch, d["ti"], d["tq"], d["steps"], d["phases"], modes=d["modes"], time_segments=e["ts"])
    if e["inmap"]:
        chain.set_input_rows(np.arange(ch) % 2, 2)
    return switch_on(chain, e)


def flavour_of(e):
    base = msdr.FLAVOUR_TAPS_PC | msdr.FLAVOUR_NCO_PC | (msdr.FLAVOUR_DECIMATED if e["kind"] == "dec" else 0)

    def f(info):
        fl = info["flavour"]
        assert fl & (msdr.FLAVOUR_TAPS_PC | msdr.FLAVOUR_OSC_PC | msdr.FLAVOUR_NCO_PC | msdr.FLAVOUR_DECIMATED | msdr.FLAVOUR_BLOCK | msdr.FLAVOUR_PREFILTER) == base, info
        assert fl & msdr.FLAVOUR_GAIN and bool(fl & msdr.FLAVOUR_COMPLEX_IN) == e["cx"], info
        assert bool(fl & msdr.FLAVOUR_METER) == e["meter"] and bool(fl & msdr.FLAVOUR_IQ_OUT) == e["iq"], info
        assert bool(fl & msdr.FLAVOUR_SHARED_IF) == e["inmap"] and bool(fl & msdr.FLAVOUR_SEGMENTED) == (e["nseg"] > 1), info
    return f


@pytest.mark.parametrize("name", cases.names(1))
def test_entry(ctx, orc, name):
    e = cases.BY_NAME[name]
    d, ch = cases.data(e), e["channels"]
    chain = make_f32(ctx, e)
    audio, pairs, meters, words = run_gain(ctx, chain, e, F, F, F64, flavour_of(e))
    chain.close()
    want = model_f32(orc, e, words, name)
    for c in range(ch):
        if c in e["unjudged"]:          # a zero gain: exact zeros, whatever the accumulators held
            assert e["gains"][c] == 0.0 and (not e["out"] or not audio[c].any()) and (not e["iq"] or not pairs[c].any()), c
        else:
            if e["out"]:
                e_go, e_gpu, e_orc = rel(audio[c], want["audio32"][c]), rel(audio[c], want["audio64"][c]), rel(want["audio32"][c], want["audio64"][c])
                print("gain census %s ch %d e_go %.3e e_gpu %.3e e_orc %.3e" % (name, c, e_go, e_gpu, e_orc))
                assert e_go < 1e-5, (name, c, e_go)
                assert e_gpu <= 2 * e_orc + 1e-6, (name, c, e_gpu, e_orc)
            if e["iq"]:
                err = rel(pairs[c], want["pairs"][c])
                print("gain census %s ch %d pairs %.3e" % (name, c, err))
                assert err < 1e-5, (name, c, err)
        if e["meter"]:          # the meter keeps the ungained pair
            meter_judged("%s ch %d" % (name, c), meters[:, c], want["meters"][:, c])
    if e["out"] and e["iq"]:
        ssb_is_the_pairs(audio, pairs, d["modes"])
    for k, (g, w) in enumerate(zip(words, want["words"])):
        for c in range(ch):
            assert np.array_equal(g[c], w[c]), (name, "call %d" % (k - 1), c, g[c].tolist(), w[c].tolist())
    assert len(words) == 4 and all(int(w[4]) == 3 * e["agc"][c] for c, w in enumerate(words[-1]))
