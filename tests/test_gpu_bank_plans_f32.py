"""The down-converter bank's host state machine under sequences nobody wrote by hand (F32): the ten fp32 plans of tests/bank_plan.py's table --
retunes, taps, input rows, D2, prefilter, complex input, held gains, meter, pairs, spectrum, init_fir / reset; half of them with the
reference's two cascade sections -- against BankModel's fp32 composition of the oracle's stages and its float64 twin.

Judged per call and receiver with the clauses the feature tests already use: audio by cx_cases.judge_f32 (e_go < 1e-5 against the fp32
composition, e_gpu <= 2 e_orc + 1e-6 against float64), pairs 1e-5, meter 2.5e-5, bins 1e-5 and power 2e-5 against float64 of the window (the
device's own pairs where a caller's d_iq holds them, as tests/test_gpu_spectrum_per_channel_f32.py does).  What is exact stays exact: statuses,
chain.nco(c), decimation(), prefilter(), complex_input(), the spectrum's cadence and count, the gain records, sentinels, the kernel family and
the flavour bits the header promises.  A twin chain runs the same plan WITHOUT its refused steps: every call of the two is bit-identical."""
import numpy as np
import pytest

import agc_model
import bank_plan as P
import cx_cases
import spectrum_model
from bank_plan_device import Device
from gpuhelp import ctx, msdr  # noqa: F401

pytestmark = pytest.mark.gpu
EXACT_BITS = {"meter": msdr.FLAVOUR_METER, "iq": msdr.FLAVOUR_IQ_OUT, "cx": msdr.FLAVOUR_COMPLEX_IN, "gain": msdr.FLAVOUR_GAIN, "spectrum": msdr.FLAVOUR_SPECTRUM,
              "prefilter": msdr.FLAVOUR_PREFILTER}


def flavour_of(m, audio_call):
    """the bits the header promises for the next call of the model's state: (must be set, must be clear)"""
    on = {k for k in EXACT_BITS if k in m.in_force()}
    must = msdr.FLAVOUR_NCO_PC | msdr.FLAVOUR_TAPS_PC | msdr.FLAVOUR_SHARED_IF          # "flavour carries MSDR_FLAVOUR_SHARED_IF while a map is in force"
    clear = 0
    for k, bit in EXACT_BITS.items():
        must, clear = (must | bit, clear) if k in on else (must, clear | bit)
    if m.plan.sections and audio_call:          # "the cascade ran behind the main kernel in CMSIS order"; in an I/Q-only call "the fp32 cascade ... do[es] not run"
        must |= msdr.FLAVOUR_SEQ_CASCADE
    else:
        clear |= msdr.FLAVOUR_SEQ_CASCADE
    if m.D2 > 1 or m.pre is not None:          # "MSDR_FLAVOUR_PREFILTER (always beside MSDR_FLAVOUR_DECIMATED ...)"
        must |= msdr.FLAVOUR_DECIMATED
    else:
        clear |= msdr.FLAVOUR_DECIMATED
    return must, clear


def same_bits(a, b):
    return (a is None and b is None) or np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("seed", P.SEEDS_F32)
def test_plan(ctx, orc, seed):
    plan = P.draw(seed, True)
    model, dev, twin = P.BankModel(plan, orc, truth=True), Device(ctx, plan), Device(ctx, plan)
    tail = spectrum_model.Tail(P.CH, np.float64)
    try:
        for i, s in enumerate(plan.steps):
            where = "step %d %r of\n%s" % (i, s, plan)
            n, cx = (model.n_samples(s), model.cx) if s[0] == "call" else (None, False)
            meter_on, iq_on, spec, was_on = model.meter, model.iq, model.spec, model.spec is not None
            must, clear = flavour_of(model, s[0] == "call" and bool(s[3]))
            want = model.apply(s)
            got = dev.apply(s, want, n, cx)
            assert got.status == want.status, (where, got.status, want.status, getattr(got, "text", ""))
            if (s[0] == "spectrum" and not was_on) or s[0] == "reset":
                tail.clear()
            if want.status == P.OK:
                ref = twin.apply(s, want, n, cx)          # the twin runs the plan without the refused steps
                assert ref.status == P.OK, where
            if s[0] == "call":
                assert got.guards, (where, "a sentinel was overwritten")
            if s[0] == "call" and want.status == P.OK:
                for name in ("audio", "pairs", "meter", "bins", "power"):
                    assert same_bits(getattr(got, name), getattr(ref, name)), (where, name, "differs from the chain that never saw the refused steps")
                assert got.kernel.startswith(want.kernel), (where, got.kernel, want.kernel)
                assert got.flavour & must == must and not got.flavour & clear, (where, hex(got.flavour), hex(must), hex(clear))
                for c in range(P.CH):
                    tag = "plan %d step %d ch %d" % (seed, i, c)
                    if want.audio_call:
                        cx_cases.judge_f32(tag, got.audio[c], want.audio[c], want.truth_audio[c])
                    if iq_on:
                        e = cx_cases.rel(got.pairs[c], want.pairs[c])
                        assert e < 1e-5, (where, c, "pairs", e)
                    if meter_on:
                        e = abs(float(got.meter[c]) - float(want.meter[c])) / float(want.meter[c])
                        assert e <= 2.5e-5, (where, c, "meter", e)
                assert got.drew == want.drew, (where, "the cadence", got.drew, want.drew)
                if spec is not None:
                    window = tail.push(got.pairs if iq_on else want.pairs)
                    if want.drew:
                        for c in range(P.CH):
                            z = spectrum_model.cfft64_f64(window[c])
                            if spec[0]:
                                b = got.bins[c].astype(np.float64)
                                ratio = float(np.sqrt(((b[:, 0] - z.real) ** 2 + (b[:, 1] - z.imag) ** 2).sum()) / np.sqrt((np.abs(z) ** 2).sum()))
                                assert ratio <= 1e-5, (where, c, "bins", ratio)
                            if spec[1]:
                                p_ref = spectrum_model.display(np.abs(z) ** 2)
                                err = float(np.abs(got.power[c].astype(np.float64) - p_ref).max() / p_ref.max())
                                assert err <= 2e-5, (where, c, "power", err)
                if model.gain_on and iq_on:          # the record's absmax from the device's own gained pairs: agc_model.Rx.absmax_of, exactly
                    for c in range(P.CH):
                        assert dev.chain.agc_state(c)["absmax"] == agc_model.Rx(True).absmax_of(got.pairs[c, :, 0], got.pairs[c, :, 1]), (where, c)
            g, w = dev.state(), model.state()
            for key in P.STATE_KEYS:
                assert g[key] == w[key], (where, key, g[key], w[key])
            if w["agc"] is None:
                assert g["agc"] is None, where
            else:          # held gains: multiplier, agc_idx, AGC_val, steps and the ring are exact (absmax above)
                for c in range(P.CH):
                    keep = np.arange(32) != 3
                    assert np.array_equal(g["agc"][c][keep], w["agc"][c][keep]), (where, "agc", c)
    finally:
        dev.close()
        twin.close()
