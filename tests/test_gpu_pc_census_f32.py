"""The census of the sliding-window per-receiver chain kernels, fp32 half: one case per fp32 entry of tests/pc_census_cases.py -- every launch
geometry pc_geometry can hand chain_f32pc_kernel (shared table, Fs/4 and FIR stage), chain_f32pco_kernel and chain_f32pcn_kernel, every CPW
instantiation of their metered, I/Q and I/Q-plus-meter twins, an input map, the tap counts around a step of 4 with all three residues of the
step count mod 3, the longest filters the setters accept, time segments (the rule's two and time_segments = 3) beside fewer than four waves,
and the long filters again behind a call that fills their history.
The recipe, the guard stretches and the reading of chain.info() are those of tests/test_gpu_pc_census.py; the flavour word is asserted too:
TAPS_PC, OSC_PC / NCO_PC, SHARED_IF, SEGMENTED, and METER / IQ_OUT exactly where set.

References and judges are the existing ones, with their present bounds and no new tolerance:
  audio   refs_of + check of tests/test_gpu_osc_per_channel_f32.py: e_go < 1e-5 and e_gpu <= 2 e_orc + fp32_noise + 1e-6 per channel over the
          three calls (tests/test_pc_census_cases.py holds every entry's bound below 5e-6 on the CPU)
  pairs   iq_ref + judged of tests/test_gpu_iq_per_channel_f32.py, per channel over the three calls
  meter   judged of tests/test_gpu_meter_per_channel_f32.py against the oracle's AM audio, per channel and call
  stage   the judge of tests/test_gpu_taps_per_channel_f32.py::test_fir_stage_per_channel: rel_rms <= 1e-6 against orclib's arm_fir_f32
and the twins' identities: audio with the tap or the meter on is bit-identical to a chain without them, the meter beside the tap is the meter
without it, LSB / USB audio is I -/+ Q of the stored pairs bit for bit, an entry with an input map is bit-identical to the same chain fed the
replicated rows.  The FIR stage (msdr_fir_f32, set_coeffs_channels) has no info call: for its entries the evidence is the oracle and the guards
alone."""
import numpy as np
import pytest

import orclib
import pc_census_cases as cases
from gpuhelp import ctx, msdr, rel_rms  # noqa: F401
from test_gpu_decim_census import raw, refusal
from test_gpu_decim_per_channel_f32 import nco_chain
from test_gpu_iq_per_channel_f32 import iq_ref, ssb_is_the_pairs
from test_gpu_iq_per_channel_f32 import judged as iq_judged
from test_gpu_meter_per_channel_f32 import judged as meter_judged
from test_gpu_osc_per_channel_f32 import check, refs_of
from test_gpu_pc_census import run_pc

pytestmark = pytest.mark.gpu
F = np.float32
_REFS = {}


def oscillator(e):
    """(osc_i, osc_q) float32 [channels, total]: the Q15 values / 32768 (exact); Fs/4: the values 0 and +-1 themselves"""
    si, sq = cases.oscillator(e, cases.total(e))
    return (si.astype(F), sq.astype(F)) if e["mixer"] == "fs4" else (cases.as_f32(si), cases.as_f32(sq))


def _cached(e, kind, build):
    k = (cases.shape_of(e), kind)
    if k not in _REFS:
        d, x = cases.data(e), cases.heard(e)
        si, sq = oscillator(e) if e["chain"] else (None, None)
        _REFS[k] = [build(d, x[c], c, si[c] if e["chain"] else None, sq[c] if e["chain"] else None) for c in range(e["channels"])]
    return _REFS[k]


def refs_f32(orc, e):
    """per channel (oracle, float64, oracle) over the three calls"""
    return _cached(e, "audio", lambda d, x, c, si, sq: refs_of(orc, x, d["modes"][c], d["ti"][c], d["tq"][c], si, sq, None))


def refs_iq(orc, e):
    """per channel (I, Q) in float64"""
    return _cached(e, "iq", lambda d, x, c, si, sq: iq_ref(orc, x, d["ti"][c], d["tq"][c], si, sq))


def refs_env(orc, e):
    """per channel the oracle's AM audio sqrt(I^2 + Q^2)"""
    return _cached(e, "env", lambda d, x, c, si, sq: orc.chain_f32(x, orclib.AM, d["ti"][c], d["tq"][c], si, sq, None))


def refs_fir(orc, e):
    """per channel orclib's arm_fir_f32 over the stream"""
    return _cached(e, "fir", lambda d, x, c, si, sq: orc.fir_f32_blocks(d["ti"][c], x, 128))


def make_f32(ctx, e, nt=None, before=False, inmap=None):
    """the entry's chain; nt: with designed rows of nt taps (part D's refusal); before: in the state before the family's last setter"""
    d, ch = cases.data(e), e["channels"]
    if nt is None:
        ti, tq = d["ti"], d["tq"]
    else:
        ti = tq = np.stack([cases.bw_taps(1, 500.0 + 350.0 * c, nt) for c in range(ch)])
    if e["mixer"] == "nco" and not before:
        chain = nco_chain(ctx, ch, ti, tq, d["steps"], d["phases"], modes=d["modes"], time_segments=e["ts"])
    else:
        if e["mixer"] == "fs4":
            chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, ti[0], tq[0], modes=d["modes"], time_segments=e["ts"])
        else:
            oi, oq = (d["oi"], d["oq"]) if d["oi"] is not None else cases.osc_rows(1, cases.ROW_LEN, seed=3)
            chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, ti[0], tq[0], mixer=msdr.MIXER_NCO, modes=d["modes"], osc_i=cases.as_f32(oi[0]), osc_q=cases.as_f32(oq[0]),
                               time_segments=e["ts"])
        if not (before and e["mixer"] in ("tab", "fs4")):
            chain.set_taps_channels_f32(0, ti, tq)
        if e["mixer"] == "rows" and not before:
            chain.set_osc_channels(0, cases.as_f32(d["oi"]), cases.as_f32(d["oq"]))
    if e["inmap"] if inmap is None else inmap:
        chain.set_input_rows(np.arange(ch) % 2, 2)
    return chain


def ask_f32(e):
    """the setter that refuses the filter one step beyond the family's limit"""
    d, ch = cases.data(e), e["channels"]
    if e["mixer"] == "rows":
        return lambda chain: chain.set_osc_channels(0, cases.as_f32(d["oi"]), cases.as_f32(d["oq"]))
    if e["mixer"] == "nco":
        return lambda chain: chain.set_nco_channels(0, d["steps"].astype(np.uint32), d["phases"].astype(np.uint32))
    rows = np.stack([cases.bw_taps(1, 500.0 + 350.0 * c, e["refuse"]) for c in range(ch)])
    return lambda chain: chain.set_taps_channels_f32(0, rows, rows)


def call_f32(ctx, chain, x):
    dy = ctx.array(x.shape, F)
    chain.process(ctx.to_device(np.ascontiguousarray(x)), dy, x.shape[1])
    return dy.download()


def fir_entry(ctx, orc, name, e):
    """the arm_fir_f32 stage with per-channel coefficients: chain_f32pc_kernel<CPW, true, false>"""
    d, ch = cases.data(e), e["channels"]
    want = refs_fir(orc, e)
    fir = msdr.FirF32(ctx, d["ti"][0], ch)
    fir.set_coeffs_channels(0, d["ti"])
    got, _, _ = run_pc(ctx, fir, e, F)
    fir.close()
    for c in range(ch):
        err = rel_rms(got[c], want[c])
        print("%s ch %d fir %.3e" % (name, c, err))
        assert err <= 1e-6, (name, c, err)


@pytest.mark.parametrize("name", cases.names(1))
def test_entry(ctx, orc, name):
    e = cases.BY_NAME[name]
    if not e["chain"]:
        fir_entry(ctx, orc, name, e)
        return
    d, x = cases.data(e), cases.heard(e)
    ch, idx = e["channels"], np.arange(cases.total(e))
    meter, iq = "meter" in e["twin"], "iq" in e["twin"]
    refs = refs_f32(orc, e)
    base = msdr.FLAVOUR_TAPS_PC | {"rows": msdr.FLAVOUR_OSC_PC, "nco": msdr.FLAVOUR_NCO_PC}.get(e["mixer"], 0)

    def flavour(with_meter, with_iq, with_map):
        def f(info):
            fl = info["flavour"]
            assert fl & (msdr.FLAVOUR_TAPS_PC | msdr.FLAVOUR_OSC_PC | msdr.FLAVOUR_NCO_PC) == base, info
            assert bool(fl & msdr.FLAVOUR_METER) == with_meter and bool(fl & msdr.FLAVOUR_IQ_OUT) == with_iq, info
            assert bool(fl & msdr.FLAVOUR_SHARED_IF) == with_map and bool(fl & msdr.FLAVOUR_SEGMENTED) == (e["nseg"] > 1), info
        return f

    def run(with_meter, with_iq, with_map=e["inmap"]):
        chain = make_f32(ctx, e, inmap=with_map)
        got = run_pc(ctx, chain, e, F, F if with_iq else None, np.float64 if with_meter else None, flavour(with_meter, with_iq, with_map),
                     replicated=e["inmap"] and not with_map)
        chain.close()
        return got

    audio, pairs, meters = run(meter, iq)
    for c in range(ch):
        check("%s ch %d" % (name, c), audio[c], x[c], refs[c], None)
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
            for n in cases.calls(e):
                want.append(e2[lo:lo + n].sum())
                lo += n
            meter_judged("%s ch %d" % (name, c), meters[:, c], np.array(want))
    if e["twin"]:          # the tap and the meter disturb nothing
        plain, _, _ = run(False, False)
        assert np.array_equal(raw(audio), raw(plain))
    if meter and iq:       # ... and the tap does not disturb the meter
        _, _, alone = run(True, False)
        assert np.array_equal(raw(meters), raw(alone))
    if e["inmap"]:         # the same chain without the map, fed the replicated rows
        rep, _, _ = run(False, False, with_map=False)
        assert np.array_equal(raw(audio), raw(rep))
    if e["refuse"] is not None:
        refusal(ctx, e, lambda nt: make_f32(ctx, e, nt, before=True), lambda chain, xs: call_f32(ctx, chain, xs), ask=ask_f32(e), x=x[:, :128])
