"""The conditions on the cases of the flavour census (tests/test_gpu_f32_flavours.py), checked without a GPU: oracle, float64 and the
library's host-side msdr_biquad_df1_f32_cascade_info only.

  * for every entry, every judged row and every judged window of a nominal run, bound = 2 e_orc + fp32_noise + 1e-6 is below the entry's
    cap -- 5e-6, half of the 1e-5 it sharpens (no entry needed a cap of its own) -- so the float64 clause is tighter than the first one;
  * the cascade removes no substantial part of its input: the contract's level, max(1, input rms / output rms), stays below 1.1 (worst
    1.048).  Exactly 1 it cannot be -- a notch removes its own band from any input -- and the census does not lean on the difference: it
    asserts e_gpu <= 2 e_orc + fp32_noise + 1e-6 with the level taken as 1;
  * no two entries name the same info() signature, and the kernel names of the table are exactly the fp32 chain kernel names that
    msdr_chain_process can report (string literals of its source): a kernel added later without a census entry turns this red;
  * the host decisions the entries rely on, by the library's criteria evaluated in float64: which cascades run in CMSIS order, which are
    too large for the matrix-product cascade's fp16 scale, which sections are row-local -- and mutant 4's case sits where only the
    float64 clause can see the mutant (tests/test_gpu_f32_teeth.py)."""
import os
import re

import numpy as np
import pytest

import test_gpu_f32_flavours as census
from f32judge import fp32_noise, level, oracle
from gpuhelp import msdr, rel_rms
from test_gpu_rowlocal_scan import _rowlocal_margin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = census.flavours(oracle())
LEVEL_CAP = 1.1          # worst over every entry, row and window: 1.048


def test_signatures_are_distinct():
    sigs = [census.signature(e) for e in ENTRIES]
    dup = sorted({s for s in sigs if sigs.count(s) > 1})
    assert dup == [], dup
    assert len({e["name"] for e in ENTRIES}) == len(ENTRIES)


def test_kernel_names_equal_those_of_msdr_chain_process():
    src = open(os.path.join(ROOT, "minimal-sdr_amd", "csrc", "msdr_api.hip")).read()
    # the names are reported by the per-path functions msdr_chain_process switches over (static int chain_launch_<path>(...)): the region
    # from the first of them to the end of msdr_chain_process, and every one of them lies inside it
    launchers = [m.start() for m in re.finditer(r"^static int chain_launch_\w+\(", src, re.M)]
    entry = src.index('extern "C" int msdr_chain_process(')
    end = entry + src[entry:].index("\n}\n")
    assert len(launchers) >= 10 and launchers[-1] < entry, launchers
    body = src[launchers[0]:end]
    assert len(re.findall(r"\bchain_launch_\w+\(c, d,", src[entry:end])) == 11       # one per path, all called from msdr_chain_process
    body = re.sub(r'launch_check\("[^"]*"\)', "", body)
    lits = {m for m in re.findall(r'"(chain_[^"]*)"', body) if "q15" not in m.lower() and not m.endswith("launch failed")}
    assert len(lits) >= 19, sorted(lits)
    mine = {e["kernel"].split(" + biquad_df1")[0] for e in ENTRIES}
    assert mine == lits, (sorted(lits - mine), sorted(mine - lits))
    suffixes = {e["kernel"][len(e["kernel"].split(" + biquad_df1")[0]):] for e in ENTRIES}
    assert suffixes == {"", " + biquad_df1_seq_kernel"}, suffixes


def test_every_template_instance_the_host_can_select_has_an_entry():
    """The launchers' switches (launch_chain_mfw / _mfb / _amtr / _fold / _generic) against the table: chain_mfw_kernel<S, AM, FOLD, FR> for
    S 0-4, both unit kinds, both layouts, FOLD for one and two sections; the two row-local kernels; chain_mfb_kernel<S, AM> for S 0-2;
    chain_fold_kernel<1|2|4>; chain_kernel<ArithF32>; chain_amtr_kernel<5, 0|1> (its other instances: unreachable)."""
    full = {("mfw", S, am, fold, fr) for S in range(5) for am in (False, True) for fold in ((False, True) if S in (1, 2) else (False,)) for fr in (False, True)}
    full |= {("mfw_rowlocal", 1), ("mfw_rowlocal", 2)} | {("mfb", S, am) for S in range(3) for am in (False, True)}
    full |= {("fold", 1), ("fold", 2), ("fold", 4), ("generic",), ("amtr", 5, 0), ("amtr", 5, 1)}
    have = set().union(*(census.instances(e) for e in ENTRIES))
    assert have == full, (sorted(map(str, full - have)), sorted(map(str, have - full)))
    src = open(os.path.join(ROOT, "minimal-sdr_amd", "csrc", "msdr_chain_stream.hip")).read() + open(os.path.join(ROOT, "minimal-sdr_amd", "csrc", "msdr_chain_block.hip")).read()
    # the switches are the ones this list was read from: five stage cases with FOLDS for 1 and 2, three block cases, three fold periods
    assert len(re.findall(r"MSDR_MFW_FOLDS\(\d\); break", src)) == 2 and len(re.findall(r"MSDR_MFW_PLAIN\(\d\); break", src)) == 3
    assert len(re.findall(r"MSDR_MFB\(\d, true\); else MSDR_MFB\(\d, false\)", src)) == 3 and len(re.findall(r"chain_fold_kernel<\d>\)", src)) == 3
    assert len(re.findall(r"chain_mfw_rowlocal_kernel<\d>\)", src)) == 2


def _model(bq):
    """msdr_chain_create's float64 model of a 1- or 2-section all-pole cascade: (decays in 8192, Rmax)."""
    S = len(bq)
    a = [(float(bq[q][3]), float(bq[q][4])) for q in range(S)]

    def run(sig, vin, n):
        y = np.zeros(n)
        for t in range(n):
            u = vin[t] if vin is not None else 0.0
            for q in range(S):
                w = u + a[q][0] * sig[2 * q] + a[q][1] * sig[2 * q + 1]
                sig[2 * q + 1] = sig[2 * q]
                sig[2 * q] = w
                u = w
            y[t] = u
        return y

    imp = np.zeros(8192)
    imp[0] = 1.0
    y = run([0.0] * 2 * S, imp, 8192)
    rmax = max(np.abs(run([1.0 if k == j else 0.0 for k in range(2 * S)], None, 32)).max() for j in range(2 * S))
    return abs(y[8191]) + abs(y[8190]) <= 1e-12, rmax


def test_host_decisions_the_entries_rely_on():
    by = {e["name"]: e for e in ENTRIES}
    for e in ENTRIES:
        if e["bq"] is None:
            continue
        seq = msdr.biquad_cascade_info(e["bq"])[2]
        # (behind the general kernel three and more sections run in CMSIS order whatever their condition: msdr_chain_create)
        forced = e["kernel"].startswith("chain_kernel<ArithF32>") and len(e["bq"]) >= 3
        assert (seq or forced) == bool(e["flavour"] & msdr.FLAVOUR_SEQ_CASCADE), (e["name"], msdr.biquad_cascade_info(e["bq"]))
        if len(e["bq"]) <= 2 and not seq:
            decays, rmax = _model(e["bq"])
            foldable = decays and rmax * 2.0 ** 14 <= 60000.0
            folded = bool(e["flavour"] & (msdr.FLAVOUR_SSB_FOLD | msdr.FLAVOUR_ENV_FOLD))
            if not (e["flavour"] & (msdr.FLAVOUR_COMPACT | msdr.FLAVOUR_VALU_FOLD)) and e["kernel"] not in ("chain_kernel<ArithF32>", "chain_amtr_kernel"):
                assert foldable == folded, (e["name"], decays, rmax * 2.0 ** 14)
    for name, s, local in (("env_s2_rowlocal_section0", 0, True), ("env_s2_rowlocal_section1", 1, True), ("env_s2_scan_4x4", 0, False), ("env_s2_scan_4x4", 1, False),
                           ("env_s2_scan1_near_threshold", 0, False), ("env_s2_scan1_near_threshold", 1, False)):
        assert (_rowlocal_margin(by[name]["bq"], s) <= 1.0) == local, (name, s)
    assert msdr.biquad_cascade_info(by["cmsis_order_behind_mfw"]["bq"])[0] > 30.0          # kCascadeConditionLimit


@pytest.mark.parametrize("name", census.FLAVOUR_NAMES)
def test_bound_is_tight_and_level_is_one(name):
    e = next(f for f in ENTRIES if f["name"] == name)
    sets, tapset, modes = census.layout(e, 4)
    ch, lens = len(modes), census.call_lengths(e)
    if e["seg"]:
        lens = [40000 + 333, 5000 + 77]          # (the conditions do not depend on where the boundaries fall: a shorter run of the same rows)
    x = census.inputs(e, ch, sum(lens))
    noise = fp32_noise(e["bq"])
    for c in census.judged_rows(e, ch):
        case = census.row_case(e, sets, tapset, modes, c)
        want, truth, pre = census.row_references(x[c], case)
        wins = census.windows(e, lens, 4, e["tile"]) if e["seg"] else census.windows(e, lens)
        for wname, w in wins:
            e_orc = rel_rms(want[w], truth[w])
            bound = 2 * e_orc + noise + 1e-6
            lvl = level(want[w], pre[w])
            print("%s row %d %-10s e_orc %.3e fp32_noise %.2e bound %.3e level %.3f" % (name, c, wname, e_orc, noise, bound, lvl))
            assert bound < 5e-6, (name, c, wname, bound)          # no entry needed a cap of its own
            assert lvl < LEVEL_CAP, (name, c, wname, lvl)


def _rowlocal_model(d, bq, n_rows_from=0):
    """What chain_mfw_rowlocal_kernel<1> computes, in float64: the cascade in the kernel's own order -- the combined numerator B0 B1 first,
    then the all-pole sections -- with section 0 entering every 32-sample row with the previous row's zero-state end value (its own
    transition over a row, M_0 sigma_0, dropped)."""
    from scipy.signal import lfilter
    b, c = [float(v) for v in bq[0]], [float(v) for v in bq[1]]
    u = lfilter(np.convolve(b[:3], c[:3]), [1.0], d)
    w = np.zeros_like(u)
    for r in range((len(u) + 31) // 32):
        lo, hi = max(0, (r - 1) * 32), min((r + 1) * 32, len(u))
        seg = lfilter([1.0], [1.0, -b[3], -b[4]], u[lo:hi])
        w[r * 32:hi] = seg[r * 32 - lo:]
    return lfilter([1.0], [1.0, -c[3], -c[4]], w)


def test_mutant_4_case_is_visible_to_the_float64_clause_only():
    """tests/test_gpu_f32_teeth.py, mutant 4: the threshold 2^-40 read as 2^-16.  At the case's Q the product build scans 4 x 4 (the criterion's
    left side is above 2^-40 of its right) and the mutant takes section 0 out of the scan (below 2^-16).  What that costs is predicted here in
    the clauses' own unit -- the relative rms distance from float64 of a float64 model of the row-local kernel on the case's own rows -- and
    must lie above 3 x the row's bound and below 1e-5 on every row, so that the 1e-5 clause passes and the float64 clause fails.  (The
    criterion's own figure, 4 Rmax mu_0 gl1[0] / gl1[1] = 4.5e-6 here, is referred to the output's bound and not to its rms, and says nothing
    about the notch's resonance, which the dropped term -- periodic with the row, 750 Hz, fourth harmonic 3000 Hz -- excites: at Q 1.5478 it
    read 9.5e-6 where the kernel measured 1.69e-5 and this model 1.70e-5.)"""
    from f32judge import truth64
    e = next(f for f in ENTRIES if f["name"] == "env_s2_scan1_near_threshold")
    term = _rowlocal_margin(e["bq"], 0) * 2.0 ** -40
    print("Q %.6f criterion's term %.3e" % (census.NEAR_Q, term))
    assert 2.0 ** -40 < term <= 2.0 ** -16
    assert 0.54 < census.NEAR_Q < 3.0
    sets, tapset, modes = census.layout(e, 4)
    n = census.call_lengths(e)[0]
    x = census.inputs(e, len(modes), sum(census.call_lengths(e)))
    for c in range(len(modes)):
        case = census.row_case(e, sets, tapset, modes, c)
        want, truth, _ = census.row_references(x[c, :n], case)
        bound = 2 * rel_rms(want, truth) + fp32_noise(e["bq"]) + 1e-6
        a = (case["hi"], case["hq"], case["oi"], case["oq"])
        predicted = rel_rms(_rowlocal_model(truth64(x[c, :n], case["mode"], *a, None), e["bq"]), truth)
        print("row %d bound %.3e predicted distance of the mutant from float64 %.3e" % (c, bound, predicted))
        assert 3 * bound < predicted < 1e-5, (c, bound, predicted)
        assert np.hypot(predicted, rel_rms(want, truth) + 1e-6) < 1e-5          # ... and from the oracle, with the oracle's own distance and the library's 1e-6 on top
