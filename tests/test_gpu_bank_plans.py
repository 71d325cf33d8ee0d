"""The down-converter bank's host state machine under sequences nobody wrote by hand (Q15): every plan of tests/bank_plan.py's table runs on a
chain of the plan's frame, and after EVERY step the device equals tests/bank_plan.py's BankModel with np.array_equal -- audio, pairs, meter,
every receiver's AGC record, PLL state, chain.nco(c), decimation(), prefilter(), complex_input(), the spectrum's count, bins and power; no
tolerance, no call and no receiver left out.  A refused step must answer with the status the header gives it and write nothing; the calls
behind it are compared like any other ("nothing changed", "nothing enqueued", "no state moved").  info()["kernel"] must begin with the
family the state implies, so that a plan cannot pass by running another path.  Every buffer a call may write carries sentinels
(tests/bank_plan_device.py).

A failure prints the plan -- one line per step, Plan.parse() reads it back -- and the step it failed at; plan.without(i) deletes a step."""
import numpy as np
import pytest

import bank_plan as P
from bank_plan_device import Device
from gpuhelp import ctx  # noqa: F401

pytestmark = pytest.mark.gpu


def same_state(got, want, where):
    for key in P.STATE_KEYS:
        assert got[key] == want[key], (where, key, got[key], want[key])
    if want["agc"] is None:
        assert got["agc"] is None, (where, "a gain record before any of the three setters")
    else:
        for c in range(P.CH):
            assert np.array_equal(got["agc"][c], want["agc"][c]), (where, "agc", c, got["agc"][c].tolist(), want["agc"][c].tolist())
    if "pll" in want:
        assert np.array_equal(got["pll"].view(np.uint32), want["pll"].view(np.uint32)), (where, "pll", got["pll"], want["pll"])


def run_plan(ctx, orc, plan):
    model, dev = P.BankModel(plan, orc), Device(ctx, plan)
    try:
        for i, s in enumerate(plan.steps):
            where = "step %d %r of\n%s" % (i, s, plan)
            n, cx = (model.n_samples(s), model.cx) if s[0] == "call" else (None, False)
            meter_on, iq_on, spec = model.meter, model.iq, model.spec
            want = model.apply(s)
            got = dev.apply(s, want, n, cx)
            assert got.status == want.status, (where, got.status, want.status, getattr(got, "text", ""))
            if s[0] == "call":
                assert got.guards, (where, "a sentinel was overwritten")
                if want.status == P.OK:
                    assert got.kernel.startswith(want.kernel), (where, got.kernel, want.kernel)
                    if want.audio_call:
                        bad = [c for c in range(P.CH) if not np.array_equal(got.audio[c], want.audio[c])]
                        assert not bad, (where, "audio of receivers", bad)
                    if iq_on:
                        assert np.array_equal(got.pairs, want.pairs), (where, "pairs")
                    if meter_on:
                        assert got.meter.dtype == np.uint64 and np.array_equal(got.meter, want.meter), (where, "meter", got.meter, want.meter)
                    assert got.drew == want.drew, (where, "the cadence", got.drew, want.drew)
                    if want.drew:
                        if spec[0]:
                            assert np.array_equal(got.bins, want.bins), (where, "bins")
                        if spec[1]:
                            assert np.array_equal(got.power.astype(np.int64), want.power), (where, "power")
            if dev.entered:          # (a plan with the bank's post passes begins with that switch, in front of the first msdr_chain_set_nco_channels)
                same_state(dev.state(), model.state(), where)
    finally:
        dev.close()


@pytest.mark.parametrize("seed", P.SEEDS_Q15)
def test_plan(ctx, orc, seed):
    run_plan(ctx, orc, P.draw(seed))

