"""The census of the decimating per-receiver chain kernels, fp32 half: one case per fp32 entry of tests/decim_census_cases.py -- every launch
geometry dec_geometry can hand chain_f32pcnd_kernel (51 keys), every (CPW, AL) instantiation of its metered, I/Q and I/Q-plus-meter twins, the
tap counts around a step of 4 and the longest filters the setter accepts.  The recipe, the guard stretches and the reading of chain.info() are
those of tests/test_gpu_decim_census.py; the flavour word is asserted too: DECIMATED | NCO_PC | TAPS_PC, and METER / IQ_OUT exactly where set.

References and judges are the existing ones, with their present bounds and no new tolerance:
  audio   refs_of + check of tests/test_gpu_osc_per_channel_f32.py, as tests/test_gpu_decim_per_channel_f32.py uses them: the FULL-RATE oracle
          and float64 streams subsampled at m D + D - 1 of every call; e_go < 1e-5 and e_gpu <= 2 e_orc + fp32_noise + 1e-6 per channel over the
          three calls (tests/test_decim_census_cases.py holds every entry's bound below 5e-6 on the CPU)
  pairs   iq_ref + judged of tests/test_gpu_iq_per_channel_f32.py, per channel over the three calls
  meter   judged of tests/test_gpu_meter_per_channel_f32.py against the oracle's AM audio, per channel and call
and the twins' identities: audio with the tap or the meter on is bit-identical to a chain without them, the meter beside the tap is the meter
without it, LSB / USB audio is I -/+ Q of the stored pairs bit for bit."""
import numpy as np
import pytest

import decim_census_cases as cases
import orclib
from gpuhelp import ctx, msdr  # noqa: F401
from test_gpu_decim_census import raw, refusal, run_entry
from test_gpu_decim_per_channel_f32 import BASE, nco_chain
from test_gpu_iq_per_channel_f32 import iq_ref, ssb_is_the_pairs
from test_gpu_iq_per_channel_f32 import judged as iq_judged
from test_gpu_meter_per_channel_f32 import judged as meter_judged
from test_gpu_nco_per_channel import Bank
from test_gpu_nco_per_channel_f32 import f32
from test_gpu_osc_per_channel_f32 import check, refs_of

pytestmark = pytest.mark.gpu
F = np.float32
_REFS = {}


def _osc(e):
    d = cases.data(e)
    si, sq = Bank(d["steps"], d["phases"]).advance(d["n"])
    return f32(si), f32(sq)


def _cached(e, kind, build):
    k = (cases.shape_of(e), kind)
    if k not in _REFS:
        d = cases.data(e)
        si, sq = _osc(e)
        _REFS[k] = [build(d, c, si[c], sq[c]) for c in range(e["channels"])]
    return _REFS[k]


def refs_f32(orc, e):
    """per channel (oracle, float64, oracle) at the outputs of the three calls"""
    idx = cases.out_index(e)
    return _cached(e, "audio", lambda d, c, si, sq: tuple(r[idx] for r in refs_of(orc, d["x"][c], d["modes"][c], d["ti"][c], d["tq"][c], si, sq, None)))


def refs_iq(orc, e):
    """per channel (I, Q) in float64 at the full rate"""
    return _cached(e, "iq", lambda d, c, si, sq: iq_ref(orc, d["x"][c], d["ti"][c], d["tq"][c], si, sq))


def refs_env(orc, e):
    """per channel the oracle's AM audio sqrt(I^2 + Q^2) at the full rate"""
    return _cached(e, "env", lambda d, c, si, sq: orc.chain_f32(d["x"][c], orclib.AM, d["ti"][c], d["tq"][c], si, sq, None))


def make_f32(ctx, e, nt=None):
    d = cases.data(e)
    ch = e["channels"]
    if nt is None:
        ti, tq = d["ti"], d["tq"]
    else:
        ti = tq = np.stack([cases.bw_taps(1, 500.0 + 350.0 * c, nt) for c in range(ch)])
    return nco_chain(ctx, ch, ti, tq, d["steps"], d["phases"], modes=d["modes"])


def call_f32(ctx, chain, x):
    dy = ctx.array(x.shape, F)
    chain.process(ctx.to_device(np.ascontiguousarray(x)), dy, x.shape[1])
    return dy.download()


@pytest.mark.parametrize("name", cases.names(1))
def test_entry(ctx, orc, name):
    e = cases.BY_NAME[name]
    d = cases.data(e)
    ch, D = e["channels"], e["D"]
    meter, iq = "meter" in e["twin"], "iq" in e["twin"]
    refs = refs_f32(orc, e)
    idx = cases.out_index(e)

    def flavour(with_meter, with_iq):
        def f(info):
            assert info["flavour"] & BASE == BASE, info
            assert bool(info["flavour"] & msdr.FLAVOUR_METER) == with_meter and bool(info["flavour"] & msdr.FLAVOUR_IQ_OUT) == with_iq, info
        return f

    def run(with_meter, with_iq):
        chain = make_f32(ctx, e)
        chain.set_decimation(D)
        assert chain.decimation() == D
        got = run_entry(ctx, chain, e, F, F if with_iq else None, np.float64 if with_meter else None, flavour(with_meter, with_iq))
        chain.close()
        return got

    audio, pairs, meters = run(meter, iq)
    for c in range(ch):
        check("%s ch %d" % (name, c), audio[c], d["x"][c], refs[c], None)
    if iq:
        ref = refs_iq(orc, e)
        for c in range(ch):
            iq_judged("%s ch %d" % (name, c), pairs[c], ref[c], idx)
        ssb_is_the_pairs(audio, pairs, d["modes"])
    if meter:
        env = refs_env(orc, e)
        for c in range(ch):
            e2 = env[c].astype(np.float64) ** 2
            lo, want = 0, []
            for nout in cases.call_outputs(e):
                want.append(e2[lo + D - 1:lo + nout * D:D].sum())
                lo += nout * D
            meter_judged("%s ch %d" % (name, c), meters[:, c], np.array(want))
    if e["twin"]:          # the tap and the meter disturb nothing
        plain, _, _ = run(False, False)
        assert np.array_equal(raw(audio), raw(plain))
    if meter and iq:       # ... and the tap does not disturb the meter
        _, _, alone = run(True, False)
        assert np.array_equal(raw(meters), raw(alone))
    if e["part"] == "D":
        refusal(ctx, e, lambda nt: make_f32(ctx, e, nt), lambda chain, x: call_f32(ctx, chain, x))
