"""msdr_chain_set_bank_post, the interface: with the switch OFF every refusal of a chain whose PLL / LMS channels would need the auxiliary
chain (fp32) or the full rate (Q15) still comes back MSDR_STATUS_ARGUMENT_ERROR with the outputs unchanged -- the existing files prove it too;
this one says it next to the switch -- and with the switch ON the same calls are accepted.  The switch's own refusals, msdr_chain_set_pll_rate's,
and graphs, which stay refused."""
import numpy as np
import pytest

import orclib
from f32pc_cases import bw_taps as bw_taps_f32, cascade
from gpuhelp import ctx, msdr  # noqa: F401
from test_gpu_nco_per_channel import any_table as any_table_q15, off_grid_steps, u32
from test_gpu_nco_per_channel_f32 import any_table as any_table_f32
from test_gpu_osc_per_channel import bw_taps as bw_taps_q15
from test_gpu_osc_per_channel_f32 import run as run_f32, signal

pytestmark = pytest.mark.gpu
B, CH = 128, 6
AM, SYNCAM = orclib.AM, orclib.SYNCAM
ARG = msdr.STATUS_ARGUMENT_ERROR
MODES = np.array([AM, SYNCAM, AM, AM, SYNCAM, AM], np.int32)
LMS = np.array([0, 1, 0, 0, 2, 0], np.int32)


def refused(f, *a, **kw):
    with pytest.raises(msdr.MsdrError) as e:
        f(*a, **kw)
    assert e.value.status == ARG, e.value
    return True


def f32_chain(ctx, pll=True, lms=False, switch=False, fs4=False, bq="lp+notch"):
    am = bw_taps_f32(2400.0)
    kw = {} if fs4 else dict(mixer=msdr.MIXER_NCO, **any_table_f32())
    chain = msdr.Chain(ctx, msdr.ARITH_F32, CH, am, am, modes=MODES, biquad_coeffs=cascade(bq) if bq else None, flags=msdr.CHAIN_SYNCAM_PLL if pll else 0, **kw)
    if lms:
        chain.set_anr(LMS)
    if switch:
        chain.set_bank_post(True)
    return chain


def q15_chain(ctx, switch=False):
    am = bw_taps_q15(2400.0)
    chain = msdr.Chain(ctx, msdr.ARITH_Q15, CH, am, am, mixer=msdr.MIXER_NCO, modes=MODES, flags=msdr.CHAIN_SYNCAM_PLL, **any_table_q15())
    if switch:
        chain.set_bank_post(True)
    return chain


def tune(rng):
    return u32(off_grid_steps(rng, CH)), u32(rng.integers(0, 1 << 32, CH, dtype=np.uint64))


def same_f32(ctx, a, b, x, tag):
    ga, gb = run_f32(ctx, a, x, B), run_f32(ctx, b, x, B)
    assert np.array_equal(ga.view(np.uint32), gb.view(np.uint32)), tag
    assert a.info() == b.info(), tag


@pytest.mark.parametrize("what", ["pll", "lms"])
def test_switch_off_an_fp32_chain_keeps_every_refusal(ctx, what):
    rng = np.random.default_rng(7300)
    steps, phases = tune(rng)
    x = signal(rng, CH, 2 * B)
    a, control = (f32_chain(ctx, pll=what == "pll", lms=what == "lms") for _ in range(2))
    assert not a.bank_post()
    a.set_bank_post(False)                                             # 0 on a chain that never had it: nothing
    meter = ctx.to_device(np.zeros(CH, np.float64))
    assert refused(a.set_nco_channels, 0, steps, phases)
    assert refused(a.set_input_rows, np.zeros(CH, np.int64), 1)
    assert refused(a.set_meter, meter)
    assert refused(a.set_biquad_coeffs_channels, 0, np.stack([cascade("lp+notch")] * CH))
    assert refused(a.set_pll_rate, 3000.0)                             # only with the switch on
    assert a.pll_rate() == 0.0
    same_f32(ctx, a, control, x, what)
    assert refused(a.set_bank_post, True)                              # samples have been processed: the history is not clear
    assert not a.bank_post()
    a.close()
    control.close()


def test_switch_off_a_q15_chain_keeps_every_refusal(ctx):
    rng = np.random.default_rng(7301)
    steps, phases = tune(rng)
    a = q15_chain(ctx)
    a.set_nco_channels(0, steps, phases)
    assert refused(a.set_decimation, 4)                                # the PLL demodulator runs at the full rate
    assert a.decimation() == 1
    a.close()
    lms = msdr.Chain(ctx, msdr.ARITH_Q15, CH, bw_taps_q15(2400.0), bw_taps_q15(2400.0), mixer=msdr.MIXER_NCO, modes=MODES, **any_table_q15())
    lms.set_nco_channels(0, steps, phases)
    lms.set_anr(LMS)
    assert refused(lms.set_decimation, 4)                              # ... and so does an LMS channel
    lms.set_anr(None, 0)
    lms.set_decimation(4)
    assert refused(lms.set_anr, LMS)                                   # ... in either order
    lms.close()


@pytest.mark.parametrize("what", ["pll", "lms", "both"])
def test_switch_on_an_fp32_chain_enters_the_mode_and_takes_every_setter(ctx, what):
    """the test that fails without the feature: each of these calls is refused on such a chain today"""
    rng = np.random.default_rng(7302)
    steps, phases = tune(rng)
    chain = f32_chain(ctx, pll=what != "lms", lms=what != "pll", switch=True)
    assert chain.bank_post()
    chain.set_bank_post(True)                                          # a repeat call does nothing
    chain.set_nco_channels(0, steps, phases)
    chain.set_input_rows(np.zeros(CH, np.int64), 1)
    meter = ctx.to_device(np.zeros(CH, np.float64))
    chain.set_meter(meter)
    chain.set_biquad_coeffs_channels(0, np.stack([cascade("lp+notch")] * CH))
    chain.set_taps_channels_f32(0, np.stack([bw_taps_f32(1500.0 + 100.0 * c) for c in range(CH)]))
    chain.set_anr(LMS)
    chain.set_mode(0, SYNCAM)
    chain.set_mode(1, AM)
    chain.set_gain(True)
    chain.set_decimation(4)
    chain.set_pll_rate(6000.0)
    assert chain.pll_rate() == 6000.0
    chain.set_pll_rate(0.0)                                            # back to the reference's constants
    x = signal(rng, 1, 4 * B)
    dy = ctx.array((CH, B), np.float32)
    chain.process(ctx.to_device(x), dy, 4 * B)
    out = dy.download()
    assert np.isfinite(out).all() and np.abs(out).max() > 1e-4
    info = chain.info()
    assert info["kernel"].startswith("chain_f32pcnd_kernel") and info["flavour"] & msdr.FLAVOUR_BANK_POST, info
    assert chain.post_kernel() == ("bank_pll_f32_kernel" if what != "lms" else "")
    assert meter.download().min() > 0
    # graphs stay refused, as on every chain in this mode
    assert refused(chain.graph, [ctx.array((1, B), np.int16) for _ in range(2)], [ctx.array((CH, B // 4), np.float32) for _ in range(2)], B)
    chain.close()


def test_switch_on_a_q15_chain_decimates_with_pll_and_lms(ctx):
    rng = np.random.default_rng(7303)
    steps, phases = tune(rng)
    chain = q15_chain(ctx, switch=True)
    chain.set_nco_channels(0, steps, phases)
    chain.set_anr(LMS)
    chain.set_decimation(4)                                            # with the PLL and LMS channels on
    chain.set_anr(LMS)                                                 # ... and while D > 1
    assert chain.decimation() == 4
    x = rng.integers(-20000, 20001, (CH, 4 * B)).astype(np.int16)
    dy = ctx.array((CH, B), np.int16)
    chain.process(ctx.to_device(x), dy, 4 * B)
    assert np.abs(dy.download().astype(np.int32)).max() > 100
    assert chain.post_kernel() == "bank_pll_q15_kernel" and chain.info()["kernel"].startswith("chain_q15pcnd_kernel")
    assert refused(chain.graph, [ctx.array((CH, B), np.int16) for _ in range(2)], [ctx.array((CH, B // 4), np.int16) for _ in range(2)], B)
    chain.close()


def test_the_switchs_own_refusals(ctx):
    rng = np.random.default_rng(7304)
    x = signal(rng, CH, B)
    # after a process call
    a = f32_chain(ctx)
    run_f32(ctx, a, x, B)
    assert refused(a.set_bank_post, True) and not a.bank_post()
    a.reset()                                                          # a clear history again
    a.set_bank_post(True)
    # 0 after 1
    assert refused(a.set_bank_post, False) and a.bank_post()
    a.close()
    # the Fs/4 mixer never enters the mode
    for chain in (f32_chain(ctx, fs4=True), msdr.Chain(ctx, msdr.ARITH_Q15, CH, bw_taps_q15(2400.0), bw_taps_q15(2400.0), modes=MODES, flags=msdr.CHAIN_SYNCAM_PLL)):
        assert refused(chain.set_bank_post, True) and not chain.bank_post()
        chain.close()
    # a chain without a PLL has no PLL state
    plain = f32_chain(ctx, pll=False)
    assert refused(plain.pll_state, 0)
    plain.close()


def test_set_pll_rate_refusals(ctx):
    for chain in (f32_chain(ctx, switch=True), q15_chain(ctx, switch=True)):
        for bad in (float("nan"), float("inf"), -3000.0, -0.5):
            assert refused(chain.set_pll_rate, bad)
            assert chain.pll_rate() == 0.0
        chain.set_pll_rate(3000.0)
        assert refused(chain.set_pll_rate, float("nan")) and chain.pll_rate() == 3000.0
        chain.set_pll_rate(0)                                          # 0: the reference's constants, the default
        assert chain.pll_rate() == 0.0
        chain.close()
    for chain in (f32_chain(ctx), q15_chain(ctx)):
        assert refused(chain.set_pll_rate, 3000.0)                     # without the switch
        chain.close()
