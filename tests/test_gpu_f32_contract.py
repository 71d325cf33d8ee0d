"""The fp32 chain's accuracy contract, as the gate sees it (include/msdr.h, next to msdr_chain_config.biquad_coeffs).

The oracle is a sequential fp32 program (oracle/msdr_oracle.c: orc_chain_f32, CMSIS order).  Behind a cascade with resonant sections
or deep stop bands ITS OWN rounding noise is a visible fraction of what is left of the signal: two correct fp32 evaluations then differ
by more than 1e-5 of the output although each is as close to the exact result as fp32 allows.  With the reference's filters and every
BASELINE configuration the library is at 5-6e-7 of the oracle; with RANDOM cascades of 1-4 sections about 3 % of the cases land
between 1e-5 and 1e-4 of the oracle (1150 of 39 940 in profiles/r03/fuzz_truth_2026_final.txt).  The contract therefore reads

        |gpu - oracle| <= 1e-5 |oracle|                                   or, where the oracle itself is that noisy,
        |gpu - f64|    <= 2 |oracle - f64| + (fp32_noise + 1e-6) |f64|    (f64: the same chain evaluated in float64, below; fp32_noise: the
                                                                          cascade's own figure from msdr_biquad_df1_f32_cascade_info -- what a
                                                                          sequential fp32 evaluation of it is from float64 on a test signal:
                                                                          4e-7 for the reference's cascade, 1e-5 for three stacked resonant
                                                                          high-passes, whose CMSIS-order evaluation answers the 5e-7 agreement
                                                                          of its INPUT with that much)
    (where the cascade removes most of its input, 1e-5 and 1e-6 are referred to the level of the cascade's INPUT: the 5e-7 agreement of
     the audio in front of the cascade is a larger fraction of what a triple high-pass leaves of it, in any fp32 evaluation)

i.e. the library may be up to twice as far from the exact result as the CMSIS order is, never more.  This file asserts exactly that
on fixed seeds -- the cases of tests/debug/fuzz_f32_truth.py (each draws from default_rng([seed, case])), including the ones the
fuzzers flagged -- so the excusal is judged by the gate and not by a debug script."""
import numpy as np
import pytest

import orclib
from f32judge import judge, truth64  # noqa: F401  (the contract's clauses and the float64 chain: shared with the flavour census)
from gpuhelp import ctx, msdr, rel_rms  # noqa: F401

pytestmark = pytest.mark.gpu
B = 128


def _case(orc, seed, case, q_max=8.0):
    """One case of tests/debug/fuzz_f32_truth.py, draw for draw."""
    rng = np.random.default_rng([seed, case])
    ntaps = int(rng.integers(2, 300))
    ch = int(rng.choice([1, 3, 40]))
    n = int(rng.integers(2, 80)) * B
    hi = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
    hq = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
    modes = rng.choice([orclib.AM, orclib.LSB, orclib.USB, orclib.CW], ch).astype(np.int32)
    if rng.integers(0, 2):
        hq = hi.copy()
    mixer = int(rng.integers(0, 2))
    P = int(rng.choice([1, 2, 4, 8, 16, 32, 64]))
    k = np.arange(B)
    if mixer:
        oi = (np.round(32767 * np.sin(2 * np.pi * k / P)).astype(np.int16) / 32768.0).astype(np.float32)
        oq = (np.round(32767 * np.cos(2 * np.pi * k / P)).astype(np.int16) / 32768.0).astype(np.float32)
    else:
        oi, oq = np.array([0, 1, 0, -1], np.float32)[k % 4], np.array([1, 0, -1, 0], np.float32)[k % 4]
    stages = int(rng.integers(1, 5))
    rows = []
    for _ in range(stages):
        kind = int(rng.choice([orclib.BQ_LOWPASS, orclib.BQ_NOTCH, orclib.BQ_HIGHPASS]))
        c_ = orc.biquad_design(kind, np.float32(rng.uniform(800, 9000)), float(rng.uniform(0.5, q_max))).astype(np.float64) / 2 ** 30
        rows.append([c_[0], c_[1], c_[2], -c_[3], -c_[4]])
    bq = np.array(rows, np.float32)
    kindx = rng.integers(0, 3)
    x = (rng.integers(-32768, 32768, (ch, n)) if kindx == 0 else rng.integers(-300, 301, (ch, n)) if kindx == 1
         else np.sign(rng.standard_normal((ch, n))) * 32767).astype(np.int16)
    segs = int(rng.choice([0, 0, 1, 3]))
    return dict(rng=rng, ntaps=ntaps, ch=ch, n=n, hi=hi, hq=hq, modes=modes, mixer=mixer, oi=oi, oq=oq, bq=bq, x=x, segs=segs, stages=stages)


def _judge(ctx, orc, cs, tag, stats):
    chain = msdr.Chain(ctx, msdr.ARITH_F32, cs["ch"], cs["hi"], cs["hq"], mixer=cs["mixer"], modes=cs["modes"],
                       osc_i=cs["oi"] if cs["mixer"] else None, osc_q=cs["oq"] if cs["mixer"] else None, biquad_coeffs=cs["bq"],
                       time_segments=cs["segs"])
    dx, dy = ctx.to_device(cs["x"]), ctx.array((cs["ch"], cs["n"]), np.float32)
    chain.process(dx, dy, cs["n"])
    got = dy.download()
    kernel = chain.info()["kernel"]
    for c in cs["rng"].choice(cs["ch"], min(cs["ch"], 3), replace=False):
        row = dict(mode=int(cs["modes"][c]), hi=cs["hi"], hq=cs["hq"], oi=cs["oi"], oq=cs["oq"], bq=cs["bq"])
        e_go, e_gpu, e_orc, bound = judge(got[c], cs["x"][c], row)       # tests/f32judge.py: the contract's clauses
        noise = msdr.biquad_cascade_info(cs["bq"])[1]
        lvl = (bound - 2 * e_orc - noise) / 1e-6                        # 1 unless a clause needed the cascade's input level
        stats["checks"] += 1
        if e_go < 1e-5:
            # The gate's TEETH (round 5): 1e-5 of the oracle is the north-star's tolerance, but the library sits at 5e-7 -- a kernel degraded
            # twentyfold (taps at 16 bits: 4e-6) would pass it.  So every case is ALSO held against float64 with the contract's second clause,
            # whether or not the first one needed excusing: never more than twice the CMSIS order's own distance from the exact result
            # (+ the cascade's fp32_noise + 1e-6 of the cascade's input level).  tests/test_gpu_f32_teeth.py shows mutated builds fail here.
            stats["tight_worst"] = max(stats.get("tight_worst", 0.0), e_gpu / bound)
            # (reported, not asserted: the same bound with the cascade's noise figure capped at the oracle's own distance -- "never more than
            #  three times as far from the exact result as the CMSIS order")
            stats["capped_worst"] = max(stats.get("capped_worst", 0.0), e_gpu / (2 * e_orc + min(noise, e_orc) + 1e-6 * lvl))
            assert e_gpu <= bound, (tag, int(c), kernel, "TIGHT clause: gpu-oracle %.2e gpu-f64 %.2e oracle-f64 %.2e level %.1f fp32_noise %.2e" % (e_go, e_gpu, e_orc, lvl, noise))
            continue
        stats["over"] += 1
        # a cascade that removes most of its input turns the 5e-7 agreement in front of it into a larger RELATIVE error of what is left (any
        # fp32 evaluation does, the oracle included): the bounds are referred to the cascade's input level there (the contract's third clause)
        if e_go < 1e-5 * lvl:
            stats["attenuating"] += 1
            continue
        stats["worst"] = max(stats["worst"], e_gpu / max(e_orc, 1e-12))
        assert e_gpu <= bound, (tag, int(c), kernel, "gpu-oracle %.2e gpu-f64 %.2e oracle-f64 %.2e level %.1f fp32_noise %.2e" % (e_go, e_gpu, e_orc, lvl, noise))
    chain.close()


def test_fp32_contract_on_the_fuzzers_cases(ctx, orc):
    """Seed 2026: cases 1 .. 150 and the flagged 39938; seeds 88 and 911 (the other two recorded runs of round 3): cases 1 .. 25 each;
    seed 4106 (round 4's run): the two cases that run flagged -- 46411, four sections whose numerators-first ORDER alone costs 11 x the
    sequential order's noise (kappa 15: every older criterion passed; the library now runs it in CMSIS order), and 34917, three resonant high-pass
    sections (kappa 7e5, fp32_noise 1e-5) that the library already runs in CMSIS order: the same arithmetic as the oracle's on an input that
    agrees to 5e-7 -- 1.1e-5 from float64 where the oracle is 4.4e-6 (the contract's fp32_noise term); seed 4206 (round 4's second pass): the five cases
    the fuzzer's first judge flagged -- two taps and a sign-only input give a CONSTANT envelope, the cascade's high-pass removes it, and what is left
    of the library's 2e-7 rounding noise (the oracle's envelope has 5 distinct values, the tiled evaluation 32) is 1.3e-5 of a decayed transient:
    the contract's input-level clause."""
    stats = dict(checks=0, over=0, worst=0.0, attenuating=0)
    for seed, cases in ((2026, list(range(1, 151)) + [39938]), (88, range(1, 26)), (911, range(1, 26)), (4106, [46411, 34917]), (4206, [9392, 12427, 16133, 19455])):
        for case in cases:
            _judge(ctx, orc, _case(orc, seed, case), (seed, case), stats)
    print("fp32 contract: %d channel checks, %d beyond 1e-5 of the fp32 oracle: %d within 1e-5 of the cascade's input level, the others judged against float64 (worst e_gpu / e_orc %.2f); "
          "every case against float64: worst e_gpu / (2 e_orc + fp32_noise + 1e-6 level) = %.2f; with fp32_noise capped at e_orc: %.2f"
          % (stats["checks"], stats["over"], stats["attenuating"], stats["worst"], stats.get("tight_worst", 0.0), stats.get("capped_worst", 0.0)))
    assert stats["checks"] >= 200
    assert stats["over"] >= 1, "no case exercised the float64 criterion: the seeds no longer reproduce the fuzzers' cases"


def test_many_sections_behind_the_general_kernel_run_in_cmsis_order(ctx, orc):
    """The one case of round 3's fuzz records that no criterion excused (profiles/r03/fuzz_kernels_606_final.txt: 277 taps behind a
    128-periodic table, four sections, chain_kernel<ArithF32>, 1.07e-5; from round 5 every 128-entry table runs on chain_mfw_kernel's full-rate
    layout whatever the tap count, and this test draws its cases behind a 96-entry table -- 96 does not divide the block, the general kernel
    answers): three or four sections behind the general kernel -- the only place where the block-parallel cascade runs with 12-sample lanes --
    now run section by section in CMSIS order."""
    rng = np.random.default_rng(606)
    k = np.arange(96)
    oi = (np.round(32767 * np.sin(2 * np.pi * k / 96)).astype(np.int16) / 32768.0).astype(np.float32)
    oq = (np.round(32767 * np.cos(2 * np.pi * k / 96)).astype(np.int16) / 32768.0).astype(np.float32)
    for trial in range(12):
        ntaps, stages = int(rng.integers(248, 500)), int(rng.integers(3, 5))
        hi = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
        hq = (rng.standard_normal(ntaps) / np.sqrt(ntaps)).astype(np.float32)
        rows = []
        for _ in range(stages):
            kind = int(rng.choice([orclib.BQ_LOWPASS, orclib.BQ_NOTCH, orclib.BQ_HIGHPASS]))
            c_ = orc.biquad_design(kind, np.float32(rng.uniform(800, 9000)), float(rng.uniform(0.5, 8))).astype(np.float64) / 2 ** 30
            rows.append([c_[0], c_[1], c_[2], -c_[3], -c_[4]])
        bq = np.array(rows, np.float32)
        x = rng.integers(-32768, 32768, (3, 33 * B)).astype(np.int16)
        chain = msdr.Chain(ctx, msdr.ARITH_F32, 3, hi, hq, mixer=msdr.MIXER_NCO, mode=orclib.USB, osc_i=oi, osc_q=oq, biquad_coeffs=bq)
        dx, dy = ctx.to_device(x), ctx.array(x.shape, np.float32)
        chain.process(dx, dy, x.shape[1])
        got = dy.download()
        assert chain.info()["kernel"] == "chain_kernel<ArithF32> + biquad_df1_seq_kernel", chain.info()["kernel"]
        for c in range(3):
            want = orc.chain_f32(x[c], orclib.USB, hi, hq, oi, oq, bq)
            e = rel_rms(got[c], want)
            if e >= 1e-5:
                t = truth64(x[c], orclib.USB, hi, hq, oi, oq, bq)
                assert rel_rms(got[c], t) <= 2 * rel_rms(want, t) + 1e-6, (trial, c, e)
        chain.close()
