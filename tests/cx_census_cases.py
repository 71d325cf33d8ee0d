"""The census of the complex-input chain kernels (minimal-sdr_amd/csrc/msdr_chain_cxpc.hiph, msdr_chain_set_complex_input): the 16 templates
chain_{q15,f32}pcn_cx[_meter|_iq|_iq_meter]_kernel<CPW> and chain_{q15,f32}pcnd_cx[_meter|_iq|_iq_meter]_kernel<CPW, AL> -- 108 instantiations,
60 Q15 and 48 fp32 -- under every launch geometry their real twins can be handed.

The table is DERIVED from the two censuses of the real-input kernels and re-derives no geometry: msdr_chain_cxpc.hiph and the two cx launchers
say that LDS, limits and read widths are the real kernels' own (tests/test_cx_census_cases.py holds them to that, from their text).  It takes
  * from tests/pc_census_cases.py every entry of the families q15pcn and f32pcn, parts A .. F: the geometry census, the twins at every CPW, with
    fewer than four waves and with a lowered CPW, the input-map entries, the tap counts, the limits with `refuse`, the calls of 4600 samples in
    time segments (ts 0 and 3) and the long filters behind a call that fills their history;
  * from tests/decim_census_cases.py every entry, parts A .. D: the 120 reachable geometries, every (CPW, AL) pair per twin and the lowered
    entries, the tap counts, the limits (those at exactly 65 536 bytes of LDS among them).
It holds no GPU code: tests/test_gpu_cx_census.py (Q15) and tests/test_gpu_cx_census_f32.py run one case per entry, tests/test_cx_census_cases.py
checks the table on the CPU.

An entry is its parent's dict (every field kept: pc_census_cases / decim_census_cases say what they mean) with
  name      "cx-" + the parent's name; unique over both halves
  parent    the parent's name;  kind: "pc" (sliding window) / "dec" (decimating)
  dir       0 / 1, alternating with the entry's position in the table: every template is met with both
and, so that one recipe reads both halves, on the decimating entries inmap = False, warm = 0, ts = 0.

The input is rows of pairs {I, Q}: I is the parent's stream x, Q a stream `xq` of the same shape and amplitude (+-30 000 for Q15, +-20 000 for
fp32), seeded by the parent's shape_of(e) and a constant of its own, so that twins of one shape share their references.  Two full-scale
streams: the Q15 sum I c +- Q s leaves int16 on some samples, the second saturation of freq_conv.cpp:67-103.  Call lengths are the parents'
(29 / 131 / 259 samples or 30 / 130 / 258 outputs, then 2, then the entry's length again): odd or no multiple of any tile, so rows of pairs
start at every dword offset modulo 4 and every entry ends in a partial tile.  With an input map the two antenna rows are rows of pairs and
channel c hears row c % 2."""
import functools

import numpy as np

import decim_census_cases as dec
import pc_census_cases as pc
from cx_cases import interleave

PC_FAMS = ("q15pcn", "f32pcn")
ARITH = dec.ARITH
TWINS = dec.TWINS
WORK_CAP = dec.WORK_CAP
XQ_SEED = 79                                       # (the parents' streams: 78 and 77)
AMP = (30000, 20000)                               # the parents' amplitudes, Q15 / fp32


def _build():
    parents = [("pc", p) for p in pc.ENTRIES if p["fam"] in PC_FAMS] + [("dec", p) for p in dec.ENTRIES]
    out = []
    for i, (kind, p) in enumerate(parents):
        e = dict(p)
        if kind == "dec":
            e.update(inmap=False, warm=0, ts=0)
        e.update(name="cx-" + p["name"], parent=p["name"], kind=kind, dir=i % 2)
        out.append(e)
    return out


ENTRIES = _build()
NAMES = [e["name"] for e in ENTRIES]
BY_NAME = {e["name"]: e for e in ENTRIES}


def names(f32):
    return [e["name"] for e in ENTRIES if e["f32"] == f32]


def parent_of(e):
    return (pc if e["kind"] == "pc" else dec).BY_NAME[e["parent"]]


def template_of(e):
    """the __global__ template of msdr_chain_cxpc.hiph the entry's launch selects"""
    return "chain_%spcn%s_cx%s_kernel" % (ARITH[e["f32"]], "d" if e["kind"] == "dec" else "", e["twin"])


def instantiation(e):
    """(template, CPW, AL): AL None for the sliding-window twins"""
    return (template_of(e), e["cpw"], e["al"] if e["kind"] == "dec" else None)


def stem(e):
    """what chain.info() names: the real kernel's stem (the names stay under msdr_chain_set_complex_input)"""
    return pc.kernel_name(e["fam"], "") if e["kind"] == "pc" else dec.kernel_name(e["f32"], "")


def work(e):
    return pc.work(e) if e["kind"] == "pc" else dec.work(e)


# ---- the entry's run ------------------------------------------------------------------------------------------------------------------------
def factor(e):
    return e["D"] if e["kind"] == "dec" else 1


def calls(e):
    """OUTPUTS of every call"""
    return pc.calls(e) if e["kind"] == "pc" else dec.call_outputs(e)


def total(e):
    """input samples of the whole stream"""
    return sum(calls(e)) * factor(e)


def out_index(e):
    """the INPUT index of every output of the calls: m D + D - 1 of each call"""
    return np.arange(total(e)) if e["kind"] == "pc" else dec.out_index(e)


def call_slices(e):
    """per call the slice of its outputs in the concatenated output"""
    out, lo = [], 0
    for m in calls(e):
        out.append(slice(lo, lo + m))
        lo += m
    return out


def shape_of(e):
    return (e["kind"],) + (pc if e["kind"] == "pc" else dec).shape_of(e)


def _seed(shape):
    if shape[0] == "pc":
        fam, mixer, osc, nt, n, ch, inmap, warm = shape[1:]
        return [XQ_SEED, 0, pc.FAM_NAMES.index(fam), pc.MIXERS.index(mixer), osc, nt, n, ch, int(inmap), warm]
    return [XQ_SEED, 1] + [int(v) for v in shape[1:]]


@functools.lru_cache(maxsize=None)
def _data(shape):
    d = dict((pc if shape[0] == "pc" else dec)._data(shape[1:]))
    f32 = pc.FAM[shape[1]]["f32"] if shape[0] == "pc" else shape[1]
    amp = AMP[f32]
    xq = np.random.default_rng(_seed(shape)).integers(-amp, amp + 1, d["x"].shape).astype(np.int16)
    d["xq"] = xq
    d["pairs"] = interleave(d["x"], xq)                                   # [rows, total, 2]: what is uploaded (the first two rows under an input map)
    d["pairs_q0"] = interleave(d["x"], np.zeros_like(xq))                 # the degenerate form's stream: Q = 0
    for k in ("xq", "pairs", "pairs_q0"):
        d[k].setflags(write=False)
    return d


def data(e):
    """the parent's data(e) (modes, taps, steps, phases, x = the I stream) and xq, pairs, pairs_q0"""
    return _data(shape_of(e))


def heard(e, x):
    """the rows of a stream x ([channels, total] or [channels, total, 2]) every channel hears"""
    return x[np.arange(e["channels"]) % 2] if e["inmap"] else x
