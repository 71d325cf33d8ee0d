"""The fp32 chain's accuracy contract (include/msdr.h) as one judge, shared by tests/test_gpu_f32_contract.py (the fuzzers' cases),
tests/test_gpu_f32_flavours.py (the census of device paths) and tests/test_f32_flavour_cases.py (the CPU-side conditions on the census's cases).

        |gpu - oracle| <= 1e-5 |oracle|                                            (first clause: the caller asserts it on e_go)
        |gpu - f64|    <= 2 |oracle - f64| + (fp32_noise + 1e-6 level) |f64|       (second clause: e_gpu <= bound)

f64 is the same chain with every operation in float64 (truth64); fp32_noise the cascade's own figure from the library's host-side
msdr_biquad_df1_f32_cascade_info; level is 1 unless the second clause fails at level 1, and then the ratio of the cascade's input level
to its output level (the third clause: a cascade that removes most of its input)."""
import numpy as np
from scipy.signal import lfilter

import orclib
from gpuhelp import msdr, rel_rms

_ORC = []


def oracle():
    if not _ORC:
        _ORC.append(orclib.Oracle())
    return _ORC[0]


def truth64(x, mode, hi, hq, oi, oq, bq):
    """orc_chain_f32 with every operation in float64."""
    n = np.arange(x.size)
    xf = x.astype(np.float64) * (1.0 / 32768)
    wi, wq = xf * oq.astype(np.float64)[n % oq.size], xf * oi.astype(np.float64)[n % oi.size]
    ai = lfilter(hi.astype(np.float64)[::-1], [1.0], wi)
    aq = lfilter(hq.astype(np.float64)[::-1], [1.0], wq)
    d = ai - aq if mode == orclib.LSB else ai + aq if mode == orclib.USB else np.sqrt(ai * ai + aq * aq)
    if bq is not None:
        for c in np.asarray(bq, np.float64):
            d = lfilter(c[:3], [1.0, -c[3], -c[4]], d)
    return d


def fp32_noise(bq):
    """What ANY sequential fp32 evaluation of this cascade is from float64 (the library's host figure; no device needed)."""
    return 0.0 if bq is None or len(bq) == 0 else float(msdr.biquad_cascade_info(np.asarray(bq, np.float32))[1])


def level(want, pre):
    """The cascade's input level over its output level, at least 1 (the contract's third clause)."""
    return max(1.0, float(np.sqrt((np.asarray(pre, np.float64) ** 2).mean() / max((np.asarray(want, np.float64) ** 2).mean(), 1e-300))))


def references(x_row, case, with_pre=True):
    """(oracle, float64, oracle without the cascade) for one input row from zero state; case: mode, hi, hq, oi, oq, bq."""
    orc = oracle()
    a = (case["hi"], case["hq"], case["oi"], case["oq"])
    want = orc.chain_f32(x_row, int(case["mode"]), *a, case["bq"])
    truth = truth64(x_row, int(case["mode"]), *a, case["bq"])
    pre = orc.chain_f32(x_row, int(case["mode"]), *a, None) if with_pre else None
    return want, truth, pre


def judge(got_row, x_row, case, refs=None, window=None):
    """-> (e_go, e_gpu, e_orc, bound).  refs: references(x_row, case) where the caller has them already (or holds rows that continue an
    earlier call's state); window: a slice of the row to judge on (segment boundaries, head, tail)."""
    want, truth, pre = refs if refs is not None else references(x_row, case, with_pre=False)
    if window is not None:
        got_row, want, truth, pre = got_row[window], want[window], truth[window], (pre[window] if pre is not None else None)
    e_go = rel_rms(got_row, want)
    e_gpu, e_orc = rel_rms(got_row, truth), rel_rms(want, truth)
    noise = fp32_noise(case["bq"])
    bound = 2 * e_orc + noise + 1e-6
    if e_gpu > bound or e_go >= 1e-5:        # the input-level clause is looked at only where a clause needs it (one more oracle pass)
        if pre is None:
            pre = references(x_row, case)[2]
            if window is not None:
                pre = pre[window]
        bound = 2 * e_orc + noise + 1e-6 * level(want, pre)
    return e_go, e_gpu, e_orc, bound
