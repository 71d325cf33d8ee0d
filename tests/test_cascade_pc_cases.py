"""The conditions on the cases of tests/test_gpu_cascade_per_channel_f32.py, checked without a GPU (oracle, float64 and the library's host-side
msdr_biquad_df1_f32_cascade_info only).  Every per-channel cascade a GPU chain test judges through f32judge gets one check here, on the very
inputs that test uses: the oracle alone stays inside the level-1 float64 clause, e_orc <= fp32_noise + 1e-6.  So the GPU tests assert the
clause at level 1 with no excused case: the share of cases a test may leave out is 0.  A family member that fails here narrows the family;
the gate is not loosened: the notches Q 15 at 400 Hz and at 1000 Hz did (the oracle 1.196e-5 from float64 against a clause of 1.142e-5, and
3.239e-6 against 3.190e-6, on the bank's own input) and are no members of the chain tests' family (tests/cascade_pc_cases.py)."""
import numpy as np
import pytest

import cascade_pc_cases as cc
import f32pc_cases as pc
from f32judge import fp32_noise, references
from gpuhelp import msdr, rel_rms


def _clause(tag, want, truth, bq):
    e_orc, noise = rel_rms(want, truth), fp32_noise(bq)
    print("%s e_orc %.3e fp32_noise %.2e clause %.3e" % (tag, e_orc, noise, noise + 1e-6))
    assert e_orc <= noise + 1e-6, (tag, e_orc, noise)


def test_the_family_is_the_designer_s():
    s = pc.sections()
    assert np.array_equal(cc.lowpass(), s["lp"]) and np.array_equal(cc.notch(3000.0, 15.0), s["notch"])
    fam = cc.family()
    assert len(fam) == 4 and len({f.tobytes() for f in fam}) == 4 and all(f.shape == (2, 5) for f in fam)
    for f in fam:
        for sec in f.astype(np.float64):
            assert abs(sec[:3].sum() / (1 - sec[3] - sec[4]) - 1.0) < 1e-3, sec                  # unit gain at DC, low-pass, notch and pass alike
        print("fp32_noise %.2e" % fp32_noise(f))
    assert any(np.array_equal(f, cc.lp_notch3k()) for f in fam)
    assert len({r.tobytes() for r in cc.bank_rows(cc.BANK_CH)}) == 4
    for stages in (1, 2, 3, 4):
        rows = cc.stage_rows(130, stages)
        assert rows.shape == (130, stages, 5) and len({r.tobytes() for r in rows}) == 6


def test_the_differential_cascade_runs_in_cmsis_order_and_the_conversion_case_block_parallel():
    assert msdr.biquad_cascade_info(cc.highpass_pair())[2] == 1
    assert msdr.biquad_cascade_info(cc.lp_notch3k())[2] == 0                                      # low-pass + notch Q 15 at 3 kHz: test 4's uniform instance


@pytest.mark.parametrize("member", range(4))
def test_bank_oracle_is_inside_the_level_one_clause(member):
    """test 7: AM, Fs/4, 102 taps; every channel of the bank that carries this family member, on the bank's own input"""
    x, rows, taps = cc.bank_input(), cc.bank_rows(cc.BANK_CH), pc.bw_taps(2400.0)
    chans = [c for c in range(cc.BANK_CH) if c % 4 == member]
    assert chans
    for c in chans:
        want, truth, _ = references(x[c], cc.case_of(cc.AM, taps, taps, rows[c]), with_pre=False)
        _clause("bank member %d ch %d" % (member, c), want, truth, rows[c])


def test_taps_and_cascade_per_channel_oracle_is_inside_the_level_one_clause():
    """test 8: 35 channels, every one its own bandwidth and its own notch"""
    x, rows, taps = cc.both_input(), cc.bank_rows(cc.BOTH_CH, 1), cc.both_taps()
    for c in range(cc.BOTH_CH):
        want, truth, _ = references(x[c], cc.case_of(cc.AM, taps[c], taps[c], rows[c]), with_pre=False)
        _clause("taps + cascade ch %d" % c, want, truth, rows[c])
    same = cc.lp_notch3k()                                                                          # the bit-identity pair's uniform cascade is judged too
    want, truth, _ = references(x[0], cc.case_of(cc.AM, taps[0], taps[0], same), with_pre=False)
    _clause("taps per channel, uniform cascade", want, truth, same)


def test_moved_cascade_oracle_is_inside_the_level_one_clause():
    """test 9: the stream whose cascade coefficients change when the first per-channel call moves the cascade behind the kernel"""
    x, m = cc.move_input(), cc.move_setup()
    for c in range(2):
        ts = m["tapsets"][c]
        plan = [(0, m["uniform"]), (2 * cc.MOVE_CALL, m["rows"][c])]
        want, truth = cc.stream_refs(x[c], m["modes"][c], m["sets_i"][ts], m["sets_q"][ts], plan)
        # the whole stream: each piece is its own cascade's fp32_noise from float64, so the stream is within the larger of the two figures
        noise_bq = max((m["uniform"], m["rows"][c]), key=fp32_noise)
        _clause("moved ch %d" % c, want, truth, noise_bq)
        _clause("moved ch %d after" % c, want[2 * cc.MOVE_CALL:], truth[2 * cc.MOVE_CALL:], m["rows"][c])


def test_df1_64_is_the_float64_cascade():
    """the float64 reference of a stream with a coefficient change, against scipy where nothing changes"""
    from scipy.signal import lfilter
    d = np.random.default_rng(5).standard_normal(700)
    bq = cc.family()[0]
    y = d
    for c in bq.astype(np.float64):
        y = lfilter(c[:3], [1.0, -c[3], -c[4]], y)
    assert rel_rms(cc.df1_64(d, [(0, bq)]), y) < 1e-12
    assert rel_rms(cc.df1_64(d, [(0, bq), (300, bq)]), y) < 1e-12
    assert rel_rms(cc.df1_64(d, [(0, bq), (300, cc.family()[3])])[300:], y[300:]) > 1e-3
