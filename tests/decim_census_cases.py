"""The census of the decimating per-receiver chain kernels (minimal-sdr_amd/csrc/msdr_chain_decpc.hiph): chain_q15pcnd_kernel / chain_f32pcnd_kernel
and their metered, I/Q and I/Q-plus-meter twins -- 8 kernel templates, each instantiated per channels-per-wave value (CPW 4 / 2 / 1) and read
width (AL; Q15 0 / 1 / 2 / 4, fp32 1 / 2 / 4) -- under every launch geometry dec_geometry (msdr_decpc_geometry.h) can hand them.

The table is BUILT FROM THE RULE as tests/test_decim_geometry.py restates it (fit, max_taps, lds_bytes), not written by hand, and holds no
GPU code: tests/test_gpu_decim_census.py (Q15) and tests/test_gpu_decim_census_f32.py run one case per entry, tests/test_decim_census_cases.py
checks the table on the CPU.  Four parts:

  A  geometry census, plain kernel.  One entry per reachable key (arithmetic, CPW class of n / D, CPW after the fit, waves, outputs per lane,
     AL): among all (D, np) that reach the key -- D 2 .. 60 / 59, np the multiples of 8 / 4 up to min(dec_max_taps, 4096) -- the one with the
     least n_out * D * np.  Call lengths 30 / 130 / 258 outputs for the classes 4 / 2 / 1: no multiple of any tile (16 .. 512), so every entry
     ends in a partial tile.
  B  twins.  For each of the six twin templates and each (CPW, AL) pair its launcher can select: the cheapest part-A shape of that pair; and
     one entry per twin at the cheapest shape whose CPW the fit lowered (from class 4: the tile is then larger than the whole call).
  C  tap counts behind D = 2, 3 and 32 at 130 outputs: np exact and padded by 1 .. 7, odd and even step counts, filters shorter than D.
  D  limits: the longest filter beside a factor (max_taps, capped at the interface's 4096), processed; `refuse` is the next padded length up.

An entry (a dict):
  name      unique; the pytest id
  part      "A" / "B" / "C" / "D"
  f32       0 Q15, 1 fp32
  twin      "" / "_meter" / "_iq" / "_iq_meter": chain_<q15|f32>pcnd<twin>_kernel
  D, nt     the factor and num_taps of the chain; np: nt padded to 8 / 4
  nout      outputs of the first and the third call (the second has SHORT = 2)
  cls       CPW by n / D alone; cpw, nw, opl: after the fit; al; lds: the workgroup's dynamic LDS by the rule; tile = opl * 64 / cpw
  channels  cpw * nw + 1, at most 17: one full workgroup and one with a single valid channel group and idle waves
  lowered   cpw < cls
  at_cap    lds == 65 536 exactly
  refuse    part D: the num_taps one step beyond the limit

`data(e)` gives the entry's channels (modes, taps, oscillator steps and phases) and its input stream, seeded by the SHAPE alone, so that twins of
one shape share their references."""
import functools

import numpy as np

import orclib
from gpuhelp import msdr
from test_decim_geometry import CAP, fit, lds_bytes, max_taps

AM, LSB, USB, CW = orclib.AM, orclib.LSB, orclib.USB, orclib.CW
ARITH = ("q15", "f32")
QUANT = (8, 4)                                     # taps per step: np is a multiple of it
MAX_D = (60, 59)                                   # MSDR_MAX_DECIMATION_Q15 / _F32
TAP_CAP = 4096                                     # msdr_chain_create: num_taps 1 .. 4096
LENGTHS = {4: 30, 2: 130, 1: 258}                  # outputs per call by CPW class
SHORT = 2                                          # outputs of the second call: n = 2 D, shorter than the history wherever np > 2 D
TWINS = ("", "_meter", "_iq", "_iq_meter")
MAX_CHANNELS = 17
WORK_CAP = 2 * 10 ** 8                             # multiply-adds of oracle work per entry
C_FACTORS = (2, 3, 32)
C_TAPS = ((2, 6, 8, 10, 16, 98, 112), (1, 2, 3, 4, 5, 7, 8, 101, 103))
D_LIMITS = (((57, 256), (58, 3968), (60, 3840), (32, 4096)), ((59, 64), (56, 256), (32, 1792)))
FIXED_STEPS = (0, 5 << 25, 0x40000000, 0xC0000000, 0xFFFFFFFF)          # tests/test_gpu_decim_per_channel.py::step_list


def kernel_name(f32, twin):
    return "chain_%spcnd%s_kernel" % (ARITH[f32], twin)


def al_of(f32, D):
    """launch_chain_q15pcnd / launch_chain_f32pcnd: the widest aligned LDS read the factor allows"""
    if f32:
        return 4 if D % 4 == 0 else 2 if D % 2 == 0 else 1
    return 0 if D & 1 else 4 if D % 8 == 0 else 2 if D % 4 == 0 else 1


def cls_of(nout):
    return 4 if nout <= 128 else 2 if nout <= 256 else 1


def padded(f32, nt):
    q = QUANT[f32]
    return (nt + q - 1) // q * q


def key_of(f32, D, np_, nout):
    """(arithmetic, CPW class, CPW, waves, outputs per lane, AL) of a launch, None where the rule refuses it"""
    g = fit(f32, np_, D, nout)
    return None if g is None else (f32, cls_of(nout), g[0], g[1], g[2], al_of(f32, D))


def reachable(nouts):
    """key -> (n_out * D * np, D, np, n_out) of the cheapest shape, over every factor and filter length the setter accepts"""
    best = {}
    for f32 in (0, 1):
        for D in range(2, MAX_D[f32] + 1):
            for np_ in range(QUANT[f32], min(max_taps(f32, D), TAP_CAP) + 1, QUANT[f32]):
                for nout in nouts:
                    cand = (nout * D * np_, D, np_, nout)
                    k = key_of(f32, D, np_, nout)
                    if k is not None and cand < best.get(k, (1 << 62,)):
                        best[k] = cand
    return best


def _entry(part, name, f32, twin, D, nt, nout, **more):
    np_ = padded(f32, nt)
    cpw, nw, opl, lds = fit(f32, np_, D, nout)
    ch = min(MAX_CHANNELS, cpw * nw + 1)
    e = dict(name=name, part=part, f32=f32, twin=twin, D=D, nt=nt, np=np_, nout=nout, cls=cls_of(nout), cpw=cpw, nw=nw, opl=opl, al=al_of(f32, D),
             lds=lds, tile=opl * (64 // cpw), channels=ch, lowered=cpw < cls_of(nout), at_cap=lds == CAP, refuse=None)
    assert lds == lds_bytes(f32, np_, D, cpw, nw, opl)
    e.update(more)
    return e


def key(e):
    return (e["f32"], e["cls"], e["cpw"], e["nw"], e["opl"], e["al"])


def work(e):
    """the oracle's multiply-adds per FIR: channels x total input samples x np"""
    return e["channels"] * (2 * e["nout"] + SHORT) * e["D"] * e["np"]


def _build():
    out = []
    best = reachable(tuple(LENGTHS.values()))
    # A
    part_a = []
    for k in sorted(best):
        f32, cls, cpw, nw, opl, al = k
        _, D, np_, nout = best[k]
        part_a.append(_entry("A", "A-%s-c%d-cpw%d-w%d-o%d-al%d-D%d-np%d" % (ARITH[f32], cls, cpw, nw, opl, al, D, np_), f32, "", D, np_, nout))
        assert key(part_a[-1]) == k
    out += part_a
    # B
    for f32 in (0, 1):
        mine = [e for e in part_a if e["f32"] == f32]
        cost = lambda e: (e["nout"] * e["D"] * e["np"], e["name"])          # noqa: E731
        for twin in TWINS[1:]:
            for cpw, al in sorted({(e["cpw"], e["al"]) for e in mine}):
                a = min((e for e in mine if (e["cpw"], e["al"]) == (cpw, al)), key=cost)
                out.append(_entry("B", "B-%s%s-cpw%d-al%d-D%d-np%d" % (ARITH[f32], twin, cpw, al, a["D"], a["np"]), f32, twin, a["D"], a["nt"], a["nout"]))
            a = min((e for e in mine if e["lowered"]), key=cost)
            out.append(_entry("B", "B-%s%s-lowered-c%d-cpw%d-al%d-D%d-np%d" % (ARITH[f32], twin, a["cls"], a["cpw"], a["al"], a["D"], a["np"]), f32, twin,
                              a["D"], a["nt"], a["nout"]))
    # C
    for f32 in (0, 1):
        for D in C_FACTORS:
            for nt in C_TAPS[f32]:
                out.append(_entry("C", "C-%s-D%d-nt%d" % (ARITH[f32], D, nt), f32, "", D, nt, LENGTHS[2]))
    # D (130 outputs: with one channel per wave and two outputs per lane a full tile and a partial one)
    for f32 in (0, 1):
        for D, nt in D_LIMITS[f32]:
            e = _entry("D", "D-%s-D%d-nt%d" % (ARITH[f32], D, nt), f32, "", D, nt, LENGTHS[2], refuse=nt + QUANT[f32])
            if e["at_cap"]:
                e["name"] += "-lds65536"
            out.append(e)
    return out


ENTRIES = _build()
NAMES = [e["name"] for e in ENTRIES]
BY_NAME = {e["name"]: e for e in ENTRIES}


def names(f32):
    return [e["name"] for e in ENTRIES if e["f32"] == f32]


# ---- the entry's run ------------------------------------------------------------------------------------------------------------------------
def call_outputs(e):
    return (e["nout"], SHORT, e["nout"])


def out_index(e):
    """the INPUT index of every output of the three calls: m D + D - 1 of each call"""
    D = e["D"]
    idx, lo = [], 0
    for m in call_outputs(e):
        idx.append(lo + D - 1 + D * np.arange(m))
        lo += m * D
    return np.concatenate(idx)


def shape_of(e):
    return (e["f32"], e["D"], e["nt"], e["nout"], e["channels"])


def bw_taps(f32, bw, nt):
    """calc_FIR_coeffs at 70 dB, as tests/test_gpu_osc_per_channel.py (Q15) and tests/f32pc_cases.py (the same rows / 32768) have it"""
    t = msdr.calc_fir_coeffs(nt, float(bw), 70.0, 0, 0.0, 24000.0)[:nt].copy()
    return (t.astype(np.float64) / 32768.0).astype(np.float32) if f32 else t


def _seeded_taps(f32, rng, nt, lo=1000, hi=12000):
    """non-zero coefficients of magnitude lo .. hi (Q15 units), for filters too short for the designer"""
    t = (rng.integers(lo, hi + 1, nt) * rng.choice([-1, 1], nt)).astype(np.int16)
    return (t.astype(np.float64) / 32768.0).astype(np.float32) if f32 else t


def _row(f32, rng, bw, nt, n_first):
    """one tap row in CMSIS order (the LAST coefficient meets the newest sample).  16 taps and more: the designer's row at bandwidth bw plus a
    seeded non-zero ripple of 1 .. 60 Q15 units on EVERY coefficient: the designer's own edge coefficients are so small that a long filter's
    first or last step could be dropped inside the fp32 clause (the census's second mutant did exactly that at 1792 taps).  A designed filter
    longer than the entry's first call would meet nothing but its own tail in a stream from the zero state (30 outputs behind D = 2 are 60
    samples under up to 3784 taps), so there the designed row has the first call's length and sits at the NEWEST end; the older coefficients
    are the ripple alone, and every tap still moves the output once its sample has arrived."""
    if nt < 16:
        return _seeded_taps(f32, rng, nt)
    m = min(nt, n_first) & ~1
    row = _seeded_taps(0, rng, nt, 1, 60)
    row[nt - m:] += bw_taps(0, bw, m)
    return (row.astype(np.float64) / 32768.0).astype(np.float32) if f32 else row


@functools.lru_cache(maxsize=None)
def _data(shape):
    f32, D, nt, nout, ch = shape
    rng = np.random.default_rng([77, f32, D, nt, nout, ch])
    steps = np.concatenate([np.array(FIXED_STEPS[:ch], np.uint64), rng.integers(0, 1 << 32, max(0, ch - len(FIXED_STEPS)), dtype=np.uint64)])
    phases = rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    modes = np.array([(AM, LSB, USB, CW)[c % 4] for c in range(ch)], np.int32)
    ti = np.stack([_row(f32, rng, 500.0 + 350.0 * c, nt, nout * D) for c in range(ch)])
    tq = np.stack([ti[c] if modes[c] == AM else _row(f32, rng, 650.0 + 350.0 * c, nt, nout * D) for c in range(ch)])
    n = (2 * nout + SHORT) * D
    amp = 20000 if f32 else 30000
    x = rng.integers(-amp, amp + 1, (ch, n)).astype(np.int16)
    for a in (steps, phases, modes, ti, tq, x):
        a.setflags(write=False)
    return dict(steps=steps, phases=phases, modes=modes, ti=ti, tq=tq, x=x, n=n)


def data(e):
    return _data(shape_of(e))
