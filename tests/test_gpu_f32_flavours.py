"""A census of the fp32 chain's device paths: every flavour a host decision in msdr_chain_create / msdr_chain_process can select is run
once, is REQUIRED to be the flavour that ran (msdr_chain_info: kernel, flavour, env_scan, time segments -- a fallback fails), and is held to
BOTH clauses of the accuracy contract (tests/f32judge.py): within 1e-5 of the fp32 oracle and within 2 e_orc + fp32_noise + 1e-6 of float64.

The fuzzers' cases (tests/test_gpu_f32_contract.py) reach whatever their draws happen to select; the table below is derived from the
template switches (launch_chain_mfw / _mfb / _amtr / _fold / _generic) and the decisions of msdr_chain_create instead.  The cases use the
reference's kinds of sections (low-pass Q 0.54, notch Q 15) and vary only what a flavour needs, so that the float64 bound stays below
5e-6 and the cascade's input-level clause is never needed: tests/test_f32_flavour_cases.py checks both on the CPU, and that the kernel
names below are exactly those msdr_chain_process can report.

Every entry: five consecutive calls (the later ones take the state over) of ragged lengths -- k tiles + 33, a call of 31 samples (shorter
than one tile and than the FIR halo), k tiles + 1, k tiles - 1, k tiles + 31; block-cadence entries 7 ticks or more (1024 samples at least); segmented entries one long call (time_segments = 4, judged
on the whole, the head, the tail and +-512 samples around every boundary) and a short one behind it.  Input rows: uniform full scale,
|x| <= 40, sign-only +-32767.  The output is pre-filled with NaN and carries a guard row.

MSDR_CENSUS_ACCURACY_ONLY=1 (set by tests/test_gpu_f32_teeth.py for the mutant whose defect changes the flavour as well, never by a plain
run) turns the info() assertion into a print, so that the child is shown to fail on accuracy."""
import os

import numpy as np
import pytest

import orclib
from f32judge import fp32_noise, judge, oracle, truth64
from gpuhelp import ctx, msdr, rel_rms  # noqa: F401
from test_gpu_rowlocal_scan import _sec

F = msdr
COS4, SIN4 = np.array([1, 0, -1, 0], np.float32), np.array([0, 1, 0, -1], np.float32)
LSB, USB, AM, CW = orclib.LSB, orclib.USB, orclib.AM, orclib.CW
NEAR_Q = 1.46              # the low-pass Q of "env_s2_scan1_near_threshold" (tests/test_gpu_f32_teeth.py, mutant 4)
MFB = " (channel-batched block tiles)"
FR = " full-rate NCO streams"


def lowpass(n, fc=2800.0):
    h = np.sinc(2 * fc / 24000 * (np.arange(n) - (n - 1) / 2)) * np.kaiser(n, 7.0)
    return (h / h.sum()).astype(np.float32)


def hilbert_pair(n, fc=1000.0, bw=1400.0):
    """A single-sideband pair (as __graft_entry__.smoke's): pass band fc +- bw / 2 of the audio, 90 degrees apart."""
    k = np.arange(n) - (n - 1) / 2
    proto = np.sinc(bw / 24000 * k) * np.kaiser(n, 6.0)
    proto /= proto.sum()
    return ((2 * proto * np.cos(2 * np.pi * fc / 24000 * k + np.pi / 4)).astype(np.float32),
            (2 * proto * np.cos(2 * np.pi * fc / 24000 * k - np.pi / 4)).astype(np.float32))


def nco(length, cycles, amp=32767):
    k = np.arange(length)
    return ((np.round(amp * np.sin(2 * np.pi * cycles * k / length)).astype(np.int16) / 32768.0).astype(np.float32),
            (np.round(amp * np.cos(2 * np.pi * cycles * k / length)).astype(np.int16) / 32768.0).astype(np.float32))


def sections(orc):
    LP, NT = orclib.BQ_LOWPASS, orclib.BQ_NOTCH
    s = dict(lp=_sec(orc, LP, 5400.0, 0.54), notch=_sec(orc, NT, 3000.0, 15.0), lpr=_sec(orc, LP, 5400.0, 6.0), lp13=_sec(orc, LP, 5400.0, 1.3),
             near=_sec(orc, LP, 5400.0, NEAR_Q),
             # state responses beyond what the matrix-product cascade's fp16 scale holds (Rmax 2^14 > 60000, float64 model in the CPU test)
             big1=_sec(orc, LP, 800.0, 3.0), big2=_sec(orc, LP, 2000.0, 6.0))
    return s


def flavours(orc):
    """The table.  Per entry: name, the configuration, and the info() it must produce: kernel, flavour, env_scan, segmented."""
    s = sections(orc)
    S0, S1, S2 = None, np.stack([s["lp"]]), np.stack([s["lp"], s["notch"]])
    S2R, S2N = np.stack([s["lpr"], s["notch"]]), np.stack([s["notch"], s["lp"]])
    S3 = np.stack([s["lp"], s["notch"], s["lp13"]])
    S4 = np.stack([s["lp"], s["lp13"], s["lp"], s["lp13"]])
    B1, B2 = np.stack([s["big1"]]), np.stack([s["big2"], s["notch"]])
    ssb, ssb160, lp100, lp100b, lp160, lp160b, lp256 = hilbert_pair(100), hilbert_pair(160), lowpass(100), lowpass(100, 2500.0), lowpass(160), lowpass(160, 2500.0), lowpass(256)
    t128 = nco(128, 5)                  # no period below 128: the full-rate layout
    t96 = nco(96, 7)                    # 96 does not divide the block: the general kernel
    t2 = (np.tile(np.array([0.5, -0.5], np.float32), 64), np.tile(np.array([1.0, -1.0], np.float32), 64))
    t1 = (np.full(128, 0.5, np.float32), np.full(128, 0.75, np.float32))
    fs4 = (np.tile(SIN4, 32), np.tile(COS4, 32))
    SSB_, ENV_, SF, EF, FRb, CP, SH, AT, BL, VF, SQ, SG = (F.FLAVOUR_SSB_UNITS, F.FLAVOUR_ENV_UNITS, F.FLAVOUR_SSB_FOLD, F.FLAVOUR_ENV_FOLD, F.FLAVOUR_FULL_RATE,
                                                           F.FLAVOUR_COMPACT, F.FLAVOUR_SHARED_IQ, F.FLAVOUR_AMTR, F.FLAVOUR_BLOCK, F.FLAVOUR_VALU_FOLD,
                                                           F.FLAVOUR_SEQ_CASCADE, F.FLAVOUR_SEGMENTED)
    P = F.FLAVOUR_FOLD_PERIOD_SHIFT
    mfw = "chain_mfw_kernel<%d>"
    mixed5 = [LSB, USB, AM, CW, AM]
    out = []

    def add(name, kernel, flavour, taps, bq, modes, osc=None, env_scan=0, tile=1024, flags=0, seg=False, block=0, sets=None):
        out.append(dict(name=name, kernel=kernel, flavour=flavour | (SG if seg else 0), env_scan=env_scan, seg=seg, taps=taps, bq=bq, modes=list(modes) if modes is not None else None, osc=osc,
                        tile=tile, flags=flags, block=block, sets=sets))

    # ---- chain_mfw_kernel<S>, SSB units (exact Fs/4 mixer, 100-tap single-sideband pair)
    add("ssb_s0", mfw % 0, SSB_, ssb, S0, [LSB, USB, LSB])
    add("ssb_s1_folded", mfw % 1, SSB_ | SF, ssb, S1, [LSB, USB, LSB])
    add("ssb_s2_folded", mfw % 2, SSB_ | SF, ssb, S2, [USB, LSB, USB])
    add("ssb_s1_not_folded", mfw % 1, SSB_, ssb, B1, [LSB, USB, LSB])
    add("ssb_s2_not_folded", mfw % 2, SSB_, ssb, B2, [LSB, USB, LSB])
    add("ssb_s3", mfw % 3, SSB_, ssb, S3, [LSB, USB, LSB])
    add("ssb_s4", mfw % 4, SSB_, ssb, S4, [LSB, USB, LSB])
    add("ssb_s2_folded_segmented", mfw % 2, SSB_ | SF, ssb, S2, [LSB, USB, LSB], seg=True)
    # ---- chain_mfw_kernel<S>, envelope units (two different low-passes: hi != hq)
    env = (lp100, lp100b)
    add("env_s0", mfw % 0, ENV_, env, S0, [AM, CW, AM])
    add("env_s1_folded", mfw % 1, ENV_ | EF, env, S1, [AM, CW, AM], env_scan=1)
    add("env_s2_scan_4x4", mfw % 2, ENV_ | EF, env, S2R, [AM, CW, AM], env_scan=1)
    add("env_s2_rowlocal_section0", mfw % 2, ENV_ | EF, env, S2, [AM, CW, AM], env_scan=2)
    add("env_s2_rowlocal_section1", mfw % 2, ENV_ | EF, env, S2N, [AM, CW, AM], env_scan=3)
    add("env_s1_not_folded", mfw % 1, ENV_, env, B1, [AM, CW, AM])
    add("env_s2_not_folded", mfw % 2, ENV_, env, B2, [AM, CW, AM])
    add("env_s3", mfw % 3, ENV_, env, S3, [AM, CW, AM])
    add("env_s4", mfw % 4, ENV_, env, S4, [AM, CW, AM])
    add("env_s2_rowlocal_segmented", mfw % 2, ENV_ | EF, env, S2, [AM, CW, AM], env_scan=2, seg=True)
    # the 4 x 4 scan, segmented, at c3's own shape (256 equal taps, Fs/4), just on the scanning side of the row-local threshold: mutant 4's case
    add("env_s2_scan1_near_threshold", mfw % 2, ENV_ | EF, (lp256, lp256), np.stack([s["near"], s["notch"]]), [AM, AM, AM], env_scan=1, seg=True)
    # ---- SSB and envelope units in one call, three tap sets, padded (-1) units in the middle and at the end of the unit table
    add("three_tapsets_mixed", mfw % 2, SSB_ | SF | ENV_ | EF, None, S2, None, env_scan=2,
        sets=[(lp100, lp100b), hilbert_pair(100, 1200.0), (lowpass(100, 2000.0), lowpass(100, 3000.0))])
    # ---- full-rate NCO streams (a 128-entry table with no shorter period)
    add("fr_ssb_s0", mfw % 0 + FR, SSB_ | FRb, ssb, S0, [LSB, USB, LSB], osc=t128)
    add("fr_ssb_s1_folded", mfw % 1 + FR, SSB_ | FRb | SF, ssb, S1, [LSB, USB, LSB], osc=t128)
    add("fr_ssb_s2_folded", mfw % 2 + FR, SSB_ | FRb | SF, ssb, S2, [LSB, USB, LSB], osc=t128)
    add("fr_ssb_s2_compact", mfw % 2 + FR, SSB_ | FRb | CP, ssb160, S2, [LSB, USB, LSB], osc=t128)
    add("fr_ssb_s4_compact", mfw % 4 + FR, SSB_ | FRb | CP, ssb160, S4, [LSB, USB, LSB], osc=t128)
    add("fr_env_s2_shared", mfw % 2 + FR, ENV_ | FRb | SH | EF, (lp100, lp100), S2, [AM, CW, AM], osc=t128, env_scan=1)
    add("fr_env_s2", mfw % 2 + FR, ENV_ | FRb | EF, env, S2, [AM, CW, AM], osc=t128, env_scan=1)
    add("fr_env_s0_compact_shared", mfw % 0 + FR, ENV_ | FRb | CP | SH, (lp160, lp160), S0, [AM, CW, AM], osc=t128)
    add("fr_env_s2_compact", mfw % 2 + FR, ENV_ | FRb | CP | EF, (lp160, lp160b), S2, [AM, CW, AM], osc=t128, env_scan=1)
    add("fr_env_s3", mfw % 3 + FR, ENV_ | FRb, env, S3, [AM, CW, AM], osc=t128)
    add("fr_ssb_s1_compact", mfw % 1 + FR, SSB_ | FRb | CP, ssb160, S1, [LSB, USB, LSB], osc=t128)
    add("fr_ssb_s3", mfw % 3 + FR, SSB_ | FRb, ssb, S3, [LSB, USB, LSB], osc=t128)
    add("fr_env_s1_folded", mfw % 1 + FR, ENV_ | FRb | EF, env, S1, [AM, CW, AM], osc=t128, env_scan=1)
    add("fr_env_s1_not_folded", mfw % 1 + FR, ENV_ | FRb, env, B1, [AM, CW, AM], osc=t128)
    add("fr_env_s2_not_folded", mfw % 2 + FR, ENV_ | FRb, env, B2, [AM, CW, AM], osc=t128)
    add("fr_env_s4", mfw % 4 + FR, ENV_ | FRb, env, S4, [AM, CW, AM], osc=t128)
    add("fr_mixed_s2_segmented", mfw % 2 + FR, SSB_ | ENV_ | FRb | SF | EF, ssb, S2, [LSB, AM, USB, CW], osc=t128, env_scan=1, seg=True)
    # ---- the taps-in-registers envelope kernel (all AM, equal taps, Fs/4, 256 taps, at most one section), alone and next to SSB units.
    # The host picks the kernel only at its largest step count and with at most one section: chain_amtr_kernel<5, 0> and <5, 1>.  The
    # instances <2..4, *> and <*, 2..4> run only with MSDR_AMTR in the environment (a test switch): unreachable, DESIGN.md 5.
    # Without a section and with one the signature is the same: the section is in this entry, none in the segmented one.
    add("amtr_s1", "chain_amtr_kernel", ENV_ | AT, (lp256, lp256), S1, [AM, CW, AM])
    add("amtr_s0_segmented", "chain_amtr_kernel", ENV_ | AT, (lp256, lp256), S0, [AM, CW, AM], seg=True)
    add("mfw_and_amtr_mixed_bank", "chain_mfw_kernel + chain_amtr_kernel", SSB_ | SF | ENV_ | AT, (lp256, lp256), S1, mixed5)
    # ---- block cadence: chain_mfb_kernel<S>
    add("mfb_env_s2_n128", "chain_mfb_kernel<2>" + MFB, BL | ENV_ | EF, env, S2, [AM, CW, AM], block=128)
    add("mfb_env_s1_n128", "chain_mfb_kernel<1>" + MFB, BL | ENV_ | EF, env, S1, [AM, CW, AM], block=128)
    add("mfb_ssb_s1_n32", "chain_mfb_kernel<1>" + MFB, BL | SSB_ | SF, ssb, S1, [LSB, USB, LSB], block=32)
    add("mfb_both_s0_n512", "chain_mfb_kernel<0>" + MFB, BL | SSB_ | ENV_, ssb, S0, mixed5, block=512)
    add("mfb_both_s2_n128", "chain_mfb_kernel<2>" + MFB, BL | SSB_ | ENV_ | SF | EF, ssb, S2, mixed5, block=128)
    # ---- the VALU fold kernel (MSDR_CHAIN_NO_MFMA), periods 1, 2, 4
    add("fold_p4", "chain_fold_kernel<4>", VF | (4 << P), ssb, S2, [LSB, AM, USB], tile=3072, flags=F.CHAIN_NO_MFMA)
    add("fold_p2", "chain_fold_kernel<2>", VF | (2 << P), ssb, S2, [LSB, USB, LSB], osc=t2, tile=3072, flags=F.CHAIN_NO_MFMA)
    add("fold_p1", "chain_fold_kernel<1>", VF | (1 << P), ssb, S1, [LSB, USB, LSB], osc=t1, tile=3072, flags=F.CHAIN_NO_MFMA)
    add("fold_p4_s0_segmented", "chain_fold_kernel<4>", VF | (4 << P), ssb, S0, [LSB, AM, USB], tile=3072, flags=F.CHAIN_NO_MFMA, seg=True)
    # ---- the general kernel (96-entry table), with and without the CMSIS-order cascade behind it
    add("generic_s2", "chain_kernel<ArithF32>", 0, ssb, S2, [LSB, AM, USB], osc=t96, tile=2560)
    add("generic_s3_cmsis_order", "chain_kernel<ArithF32> + biquad_df1_seq_kernel", SQ, ssb, S3, [LSB, AM, USB], osc=t96, tile=2560)
    add("generic_s0_segmented", "chain_kernel<ArithF32>", 0, ssb, S0, [LSB, AM, USB], osc=t96, tile=2560, seg=True)
    # ---- a cascade over kCascadeConditionLimit behind a matrix-core kernel: the reference's notch ALONE has kappa 57 (its poles are not
    # cancelled by a low-pass's roll-off) and fp32_noise 4.5e-7 -- the bound stays under the common cap, no entry needs one of its own
    add("cmsis_order_behind_mfw", "chain_mfw_kernel<0> + biquad_df1_seq_kernel", SSB_ | ENV_ | SQ, ssb, np.stack([s["notch"]]), [LSB, AM, USB])
    for e in out:
        if e["osc"] is None:
            e["osc"], e["mixer"] = fs4, msdr.MIXER_FS4
        else:
            e["mixer"] = msdr.MIXER_NCO
    return out


FLAVOUR_NAMES = [e["name"] for e in flavours(oracle())]


def signature(e):
    return (e["kernel"], e["flavour"], e["env_scan"], bool(e["seg"]))


def instances(e):
    """The template instances an entry's launches select, by the switches of launch_chain_mfw / _mfb / _amtr / _fold / _generic read against
    what msdr_chain_process passes them: a set of tuples.  tests/test_f32_flavour_cases.py holds the union against the full product."""
    f, k, out = e["flavour"], e["kernel"], set()
    stages = 0 if e["bq"] is None or (f & F.FLAVOUR_SEQ_CASCADE) else len(e["bq"])          # (a CMSIS-order cascade is not in the main kernel)
    if f & F.FLAVOUR_VALU_FOLD:
        return {("fold", (f >> F.FLAVOUR_FOLD_PERIOD_SHIFT) & 7)}
    if k.startswith("chain_kernel<ArithF32>"):
        return {("generic",)}
    for am, units, fold in ((False, F.FLAVOUR_SSB_UNITS, F.FLAVOUR_SSB_FOLD), (True, F.FLAVOUR_ENV_UNITS, F.FLAVOUR_ENV_FOLD)):
        if not f & units:
            continue
        if f & F.FLAVOUR_BLOCK:
            out.add(("mfb", stages, am))
        elif am and f & F.FLAVOUR_AMTR:
            out.add(("amtr", 5, stages))
        elif am and e["env_scan"] >= 2:
            out.add(("mfw_rowlocal", e["env_scan"] - 1))
        else:
            out.add(("mfw", stages, am, bool(f & fold), bool(f & F.FLAVOUR_FULL_RATE)))
    return out


def layout(e, nw=4):
    """-> (tap sets [(hi, hq)], per-channel tap set, per-channel mode).  The three-set entry: per set 1, nw - 1 and nw + 1 channels of the
    wave-stream kernel's workgroup size, so that the unit table is padded inside and at its end."""
    if e["sets"] is None:
        return [e["taps"]], [0] * len(e["modes"]), e["modes"]
    tapset, modes = [], []
    for k, cnt in enumerate([1, max(nw - 1, 1), nw + 1]):
        tapset += [k] * cnt
        modes += [[AM, LSB, CW], [USB, AM, LSB], [LSB, USB, AM]][k][:cnt] + [AM if (k + j) & 1 else USB for j in range(max(cnt - 3, 0))]
    return e["sets"], tapset, modes


def call_lengths(e):
    if e["block"]:
        return [e["block"]] * max(7, 1024 // e["block"])
    if e["seg"]:
        return [150000 + 333, 5000 + 77]
    t = e["tile"]
    return [2 * t + 33, 31, t + 1, 2 * t - 1, t + 31]          # every edge in every entry; each later call takes the state over


def inputs(e, ch, n):
    """Row kinds in turn: uniform full scale, |x| <= 40, sign-only +-32767 (no entry leaves one out)."""
    rng = np.random.default_rng([4242, len(e["name"]), sum(map(ord, e["name"]))])
    x = np.empty((ch, n), np.int16)
    for c in range(ch):
        x[c] = (rng.integers(-32768, 32768, n) if c % 3 == 0 else rng.integers(-40, 41, n) if c % 3 == 1 else np.where(rng.integers(0, 2, n) > 0, 32767, -32767)).astype(np.int16)
    return x


def judged_rows(e, ch):
    if ch <= 8:
        return list(range(ch))
    rng = np.random.default_rng(len(e["name"]))
    return sorted({0, ch - 1} | set(int(v) for v in rng.choice(np.arange(1, ch - 1), 3, replace=False)))


def row_case(e, sets, tapset, modes, c):
    hi, hq = sets[tapset[c]]
    return dict(mode=int(modes[c]), hi=hi, hq=hq, oi=e["osc"][0], oq=e["osc"][1], bq=e["bq"])


def row_references(x_row, case):
    """(oracle, float64, oracle without cascade) over the whole stream of an entry's consecutive calls."""
    orc = oracle()
    a = (case["hi"], case["hq"], case["oi"], case["oq"])
    return (orc.chain_f32(x_row, case["mode"], *a, case["bq"]), truth64(x_row, case["mode"], *a, case["bq"]), orc.chain_f32(x_row, case["mode"], *a, None))


def windows(e, lens, info_segments=None, info_tile=None):
    """What is judged: every call on its own; for a segmented first call also its head, its tail and +-512 samples around each boundary."""
    w, o = [], 0
    if e["block"]:                      # a tick is too short to be judged alone while the FIR fills: the whole run, and its last tick
        return [("all", slice(0, sum(lens))), ("last_tick", slice(sum(lens) - lens[-1], sum(lens)))]
    for k, n in enumerate(lens):
        lo = o - lens[k - 1] if k and lens[k - 1] < 64 else o
        if n >= 64:                     # 31 samples are no sample of an rms: that call is judged together with the one behind it
            w.append(("call%d" % k if lo == o else "call%d+%d" % (k - 1, k), slice(lo, o + n)))
        o += n
    if e["seg"] and info_segments and info_segments > 1:
        n = lens[0]
        seg = -(-n // info_segments)
        seg = -(-seg // info_tile) * info_tile
        w += [("head", slice(0, 2048)), ("tail", slice(n - 1500, n))]
        for sgm in range(1, info_segments):
            if sgm * seg + 64 <= n:
                w.append(("boundary%d" % sgm, slice(sgm * seg - 512, sgm * seg + 512)))
    return w


pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", FLAVOUR_NAMES)
def test_flavour_runs_and_meets_both_clauses(ctx, orc, name):
    e = next(f for f in flavours(orc) if f["name"] == name)
    accuracy_only = os.environ.get("MSDR_CENSUS_ACCURACY_ONLY") == "1"
    nw = 4
    if e["sets"] is not None:           # the workgroup size the host picks for these tables (a one-channel chain of the same tables says it)
        probe = msdr.Chain(ctx, msdr.ARITH_F32, 1, [s_[0] for s_ in e["sets"]], [s_[1] for s_ in e["sets"]], mixer=e["mixer"], mode=AM, biquad_coeffs=e["bq"])
        dx, dy = ctx.to_device(np.zeros((1, 2048), np.int16)), ctx.array((1, 2048), np.float32)
        probe.process(dx, dy, 2048)
        nw = probe.info()["block"] // 64
        probe.close()
        assert nw >= 2, nw
    sets, tapset, modes = layout(e, nw)
    ch, lens = len(modes), call_lengths(e)
    x = inputs(e, ch, sum(lens))
    chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, [s_[0] for s_ in sets], [s_[1] for s_ in sets], mixer=e["mixer"], modes=np.array(modes, np.int32),
                       tapsets=np.array(tapset, np.int32), osc_i=e["osc"][0] if e["mixer"] == msdr.MIXER_NCO else None,
                       osc_q=e["osc"][1] if e["mixer"] == msdr.MIXER_NCO else None, biquad_coeffs=e["bq"], time_segments=4 if e["seg"] else 0, flags=e["flags"])
    got = np.empty((ch, sum(lens)), np.float32)
    o, first_info = 0, None
    for k, n in enumerate(lens):
        dx = ctx.to_device(np.ascontiguousarray(x[:, o:o + n]))
        dy = ctx.to_device(np.full((ch + 1, n), np.nan, np.float32))                 # NaN everywhere, one guard row behind the last channel
        chain.process(dx, dy, n)
        y = dy.download()
        assert np.isnan(y[ch]).all(), (name, k, "the guard row behind the last channel was written")
        assert not np.isnan(y[:ch]).any(), (name, k, "NaN left in the output", np.argwhere(np.isnan(y[:ch]))[:4])
        got[:, o:o + n] = y[:ch]
        o += n
        info = chain.info()
        if k == 0:
            first_info = info
        want_sig = (e["kernel"], e["flavour"], e["env_scan"], bool(e["seg"]) and k == 0)
        have_sig = (info["kernel"], info["flavour"], info["env_scan"], info["time_segments"] > 1)
        if e["seg"] and k > 0:            # the short call behind a segmented one is one segment: the same flavour without that bit
            want_sig = (e["kernel"], e["flavour"] & ~F.FLAVOUR_SEGMENTED, e["env_scan"], False)
        print(name, "call", k, n, info)
        if accuracy_only:
            if have_sig != want_sig:
                print(name, "FLAVOUR DIFFERS (accuracy only: not asserted)", have_sig, want_sig)
        else:
            assert have_sig == want_sig, (name, k, have_sig, want_sig)
        if e["seg"] and k == 0 and not accuracy_only:
            assert info["time_segments"] >= 3, info             # boundaries to judge: the four segments asked for, three at the least
    chain.close()
    worst = 0.0
    for c in judged_rows(e, ch):
        case = row_case(e, sets, tapset, modes, c)
        refs = row_references(x[c], case)
        noise = fp32_noise(e["bq"])
        for wname, w in windows(e, lens, first_info["time_segments"], first_info["tile"]):
            e_go, e_gpu, e_orc, bound = judge(got[c], x[c], case, refs=refs, window=w)
            b1 = 2 * e_orc + noise + 1e-6                               # level 1: no entry may need the input-level clause
            worst = max(worst, e_gpu / b1)
            print("%s row %d %-10s e_go %.3e e_gpu %.3e e_orc %.3e bound %.3e ratio %.2f" % (name, c, wname, e_go, e_gpu, e_orc, b1, e_gpu / b1))
            assert e_go < 1e-5, (name, c, wname, "first clause", e_go)
            assert e_gpu <= min(bound, b1), (name, c, wname, "float64 clause: e_gpu %.3e e_orc %.3e fp32_noise %.2e bound %.3e" % (e_gpu, e_orc, noise, b1))
    print("CENSUS %s worst e_gpu / bound %.3f" % (name, worst))
