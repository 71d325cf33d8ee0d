"""The envelope flavour of the wave-stream chain (256-tap AM tables, two-section cascade as matrix products) scans the cascade's row
states either with 4 x 4 matrices or -- where one section's transition over a 32-sample row is nothing in fp32 -- leaves that section
out of the scan and runs the other one alone with 2 x 2 matrices (chain_mfw_rowlocal_kernel, msdr_chain_mfw.hiph).  The host decides at
create and at every coefficient rewrite.  Here: both scans against the sequential oracle (head from zero state, the time-segment
boundaries, the tail, a second call that takes the state over), the decision on either side of its threshold, and a cascade rewritten
damped -> resonant -> damped under a running stream.  msdr_chain_info.env_scan says which scan ran: 1 = every section, 2 / 3 = section
0 / 1 row-local; a test cannot pass by falling back to the other one."""
import os
import subprocess

import numpy as np
import pytest

import orclib
from gpuhelp import ctx, msdr, rel_rms  # noqa: F401
from test_gpu_chain import run_chain, CORR

pytestmark = pytest.mark.gpu
TOL = 1e-5
COS4, SIN4 = np.array([1, 0, -1, 0], np.float32), np.array([0, 1, 0, -1], np.float32)
NTAPS = 256


def _lowpass256():
    lp = (np.sinc(2 * 2800 / 24000 * (np.arange(NTAPS) - (NTAPS - 1) / 2)) * np.kaiser(NTAPS, 7.0)).astype(np.float32)
    return (lp / lp.sum()).astype(np.float32)


def _sec(orc, kind, f, q):
    c = orc.biquad_design(kind, np.float32(f * CORR), q).astype(np.float64) / 2 ** 30
    return np.array([c[0], c[1], c[2], -c[3], -c[4]], np.float32)


def _rowlocal_margin(bq, s):
    """The library's criterion in float64 (msdr_chain_create): section s of a two-section cascade is row-local when
    4 Rmax mu_s gl1[s] <= 2^-40 gl1[1]; returns left / right (<= 1: row-local)."""
    a = [(float(bq[q][3]), float(bq[q][4])) for q in range(2)]

    def run(sig, vin, n, upto=1):
        y = np.zeros(n)
        for t in range(n):
            u = vin[t] if vin is not None else 0.0
            for q in range(upto + 1):
                w = u + a[q][0] * sig[2 * q] + a[q][1] * sig[2 * q + 1]
                sig[2 * q + 1] = sig[2 * q]
                sig[2 * q] = w
                u = w
            y[t] = u
        return y

    imp = np.zeros(8192)
    imp[0] = 1.0
    gl1 = [np.abs(run([0.0] * 4, imp, 8192, upto=q)).sum() for q in range(2)]
    rmax = max(np.abs(run([1.0 if k == j else 0.0 for k in range(4)], None, 32)).max() for j in range(4))
    m = np.linalg.matrix_power(np.array([[a[s][0], a[s][1]], [1.0, 0.0]]), 32)
    return 4.0 * rmax * np.abs(m).max() * gl1[s] / (2.0 ** -40 * gl1[1])


def _lowpass_q_at_margin(orc, other, target):
    """Q of the 5400 Hz low-pass (section 0, next to `other`) at which the criterion's left / right is `target`, by bisection: the pole
    radius grows with Q (0.21 at the reference's 0.54, about 0.43 at the threshold)."""
    lo, hi = 0.54, 3.0
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        if _rowlocal_margin([_sec(orc, orclib.BQ_LOWPASS, 5400.0, mid), other], 0) <= target:
            lo = mid
        else:
            hi = mid
    return lo


def _cases(orc):
    lp, notch = _sec(orc, orclib.BQ_LOWPASS, 5400.0, 0.54), _sec(orc, orclib.BQ_NOTCH, 3000.0, 15.0)
    lpr = _sec(orc, orclib.BQ_LOWPASS, 5400.0, 6.0)             # (resonant, and its state response small enough for the matrix-product cascade)
    q_below, q_above = _lowpass_q_at_margin(orc, notch, 0.4), _lowpass_q_at_margin(orc, notch, 2.5)
    return {
        "c3_lowpass_notch": (np.stack([lp, notch]), 2),
        "notch_lowpass": (np.stack([notch, lp]), 3),
        "one_damped_section": (np.stack([lp]), None),
        "two_resonant": (np.stack([lpr, notch]), 1),
        "just_below_threshold": (np.stack([_sec(orc, orclib.BQ_LOWPASS, 5400.0, q_below), notch]), 2),
        "just_above_threshold": (np.stack([_sec(orc, orclib.BQ_LOWPASS, 5400.0, q_above), notch]), 1),
    }


CASE_NAMES = ["c3_lowpass_notch", "notch_lowpass", "one_damped_section", "two_resonant", "just_below_threshold", "just_above_threshold"]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_rowlocal_and_full_scan_against_the_oracle(ctx, orc, name):
    bq, scan = _cases(orc)[name]
    if name.startswith("just_"):       # the two sides of the threshold are what they claim, by the criterion in float64
        mg = _rowlocal_margin(bq, 0)
        print(name, "criterion left/right =", mg)
        assert (mg < 1.0) == (scan == 2) and 0.2 < mg < 5.0, mg
    rng = np.random.default_rng(len(name))
    ch, n, n2 = 2, 150000 + 333, 5000 + 77
    lp = _lowpass256()
    x = rng.integers(-12000, 12001, (ch, n + n2)).astype(np.int16)
    chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, lp, lp, mixer=msdr.MIXER_FS4, mode=orclib.AM, biquad_coeffs=bq, time_segments=4)
    got = run_chain(ctx, chain, x[:, :n], np.float32)
    info = chain.info()
    print(name, info)
    if scan is None:
        assert info["env_scan"] in (0, 1), info                 # a single section has nothing to leave out of its scan
    else:
        assert info["kernel"].startswith("chain_mfw_kernel<2>") and info["env_scan"] == scan, info
        assert info["time_segments"] > 1 and info["warmup"] > 0, info
    got2 = run_chain(ctx, chain, x[:, n:], np.float32)           # a second call: the state hand-off of the first
    seg = -(-n // info["time_segments"])
    seg = -(-seg // info["tile"]) * info["tile"]
    for c in range(ch):
        st = {}
        want = orc.chain_f32(x[c, :n], orclib.AM, lp, lp, SIN4, COS4, bq, state=st)
        want2 = orc.chain_f32(x[c, n:], orclib.AM, lp, lp, SIN4, COS4, bq, state=st)
        errs = {"all": rel_rms(got[c], want), "head": rel_rms(got[c, :2048], want[:2048]), "tail": rel_rms(got[c, -1500:], want[-1500:]),
                "second_call": rel_rms(got2[c], want2)}
        for s in range(1, info["time_segments"]):
            lo = s * seg
            if lo + 64 <= n:
                errs["boundary%d" % s] = rel_rms(got[c, lo - 512:lo + 512], want[lo - 512:lo + 512])
        print(name, c, errs)
        for k, e in errs.items():
            assert e < TOL, (name, c, k, e)


def test_cascade_rewritten_damped_resonant_damped_under_a_running_stream(ctx, orc):
    lpd, notch = _sec(orc, orclib.BQ_LOWPASS, 5400.0, 0.54), _sec(orc, orclib.BQ_NOTCH, 3000.0, 15.0)
    lpr = _sec(orc, orclib.BQ_LOWPASS, 5400.0, 6.0)             # (resonant, and its state response small enough for the matrix-product cascade)
    plan = [(np.stack([lpd, notch]), 2), (np.stack([lpr, notch]), 1), (np.stack([lpd, notch]), 2), (np.stack([notch, lpd]), 3), (np.stack([lpd, notch]), 2)]
    rng = np.random.default_rng(77)
    ch = 3
    lp = _lowpass256()
    chain = msdr.Chain(ctx, msdr.ARITH_F32, ch, lp, lp, mixer=msdr.MIXER_FS4, mode=orclib.AM, biquad_coeffs=plan[0][0])
    states = {c: {} for c in range(ch)}
    for k, (bq, scan) in enumerate(plan):
        if k:
            chain.set_biquad_coeffs(bq)
        x = rng.integers(-12000, 12001, (ch, 3000 + 1111 * k)).astype(np.int16)
        got = run_chain(ctx, chain, x, np.float32)
        info = chain.info()
        assert info["kernel"].startswith("chain_mfw_kernel<2>") and info["env_scan"] == scan, (k, info)
        for c in range(ch):
            want = orc.chain_f32(x[c], orclib.AM, lp, lp, SIN4, COS4, bq, state=states[c])
            e = rel_rms(got[c], want)
            print("rewrite", k, c, e)
            assert e < TOL, (k, c, e)


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "minimal-sdr_amd", "lib", "libmsdr.so")
OBJDUMP, READELF = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"


@pytest.mark.skipif(not (os.path.exists(OBJDUMP) and os.path.exists(READELF)), reason="llvm-objdump / llvm-readelf missing")
def test_rowlocal_kernels_keep_128_registers_and_no_scratch(tmp_path):
    """As tests/test_chain_kernel_no_scratch.py asks of chain_mfw_kernel: both row-local kernels at <= 128 registers, no scratch instruction."""
    subprocess.run(["cp", LIB, str(tmp_path / "libmsdr.so")], check=True)
    subprocess.run([OBJDUMP, "--offloading", "libmsdr.so"], cwd=tmp_path, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    seen = 0
    for co in sorted(f for f in os.listdir(tmp_path) if "gfx950" in f):
        notes = subprocess.run([READELF, "--notes", co], cwd=tmp_path, check=True, stdout=subprocess.PIPE, text=True).stdout
        for block in notes.split(".name:")[1:]:
            if "chain_mfw_rowlocal_kernel" not in block.split()[0]:
                continue
            seen += 1
            f = {k: int(v) for k, v in __import__("re").findall(r"\.(vgpr_count|agpr_count|private_segment_fixed_size|vgpr_spill_count):\s+(\d+)", block)}
            assert f["vgpr_count"] + f.get("agpr_count", 0) <= 128 and f["private_segment_fixed_size"] == 0 and f.get("vgpr_spill_count", 0) == 0, (block.split()[0], f)
    assert seen == 2, seen
