"""The census of the two-stage decimating per-receiver chain kernels (minimal-sdr_amd/csrc/msdr_chain_pre.hiph, msdr_chain_set_prefilter):
chain_q15pcn2[_full]_kernel<CPW 1 / 2 / 4, AL 0 / 1 / 2 / 4> and chain_f32pcn2[_full]_kernel<CPW 1 / 2 / 4, AL 1 / 2 / 4> -- 42 kernels -- under
every launch geometry pre_geometry (msdr_prepc_geometry.h) can hand them, with every stage-1 read width (chosen at run time by D1) at every
count of lanes per channel.

The table is BUILT FROM THE RULE as tests/prefilter_model.py restates it (fits, geometry, lds_bytes, chunk), not written by hand, and holds no
GPU code: tests/test_gpu_pre_census.py (Q15) and tests/test_gpu_pre_census_f32.py run one case per entry, tests/test_pre_census_cases.py checks
the table on the CPU.  Six parts:

  A  geometry census, plain kernel.  One entry per reachable key (arithmetic, CPW class of n_out, CPW after the fit, waves, outputs per lane,
     AL of D2).  The search: D1 2 .. 32, np1 = q, 4 q, 16 q, ... (q: 8 / 4 taps per step; the cheapest shape of a key always has a short
     prefilter, which costs D1 times a channel tap's work and less than half its LDS), np2 every multiple of q up to 4096, D2 1 .. 60 / 59;
     only shapes whose stream is at least as long as both filters (every tap meets a sample in a stream from the clear state); the cost is the
     oracle's multiply-adds.  D1 ROTATES over the keys of one (arithmetic, CPW), so that each of the 30 triples (arithmetic, D1, CPW) occurs:
     every stage-1 loop at every lane count; a key takes the cheapest shape of its turn's D1.
  B  the _full twins.  For each arithmetic and each (CPW, AL) its launcher can select (12 + 9) the cheapest part-A shape of the pair on the
     twin, the parts switched on rotating through the seven non-empty subsets of {meter, pairs, gain} (fixed per-channel gains, AGC off); the
     first entry with the pairs alone on makes I/Q-only calls (a null audio pointer); one entry whose CPW the fit lowered; one with AGC on.
  C  prefilter lengths behind D1 = 2, 16, 32 at 130 outputs, (N2, D2) = (24, 3) (Q15: two copies of the window): N1 exact and front-padded by
     every amount the step allows, N1 < D1; at D1 = 16 a window that is a whole number of chunks (N2 = 32) and one whose last chunk holds a
     single step of intermediates (N2 = 8 / 4: the window's length is a multiple of the step, so a lone intermediate cannot occur).
  D  limits.  N1 = pre_max_taps beside two (D1, np2, D2), processed, `refuse` one step longer; D2 = pre_max_decimation beside two
     (np1, D1, np2), processed, `refuse` = D2 + 1.  An entry whose LDS is exactly 65 536 bytes says so.
  E  stage-1 arithmetic edges, Q15: full-scale rows at oscillator step 0 through a prefilter with sum |p| = 462 000, at every D1.
  F  time segments, CPW 1: ONE call of 8 tiles + 2 outputs per arithmetic and tile (outputs per lane 2, 4, 8): two segments of five tiles, the
     last of which lies wholly past n_out.

An entry (a dict):
  name      unique; the pytest id
  part      "A" .. "F"
  f32       0 Q15, 1 fp32
  full      the _full twin runs (any of meter / iq / gain set); meter, iq, gain, agc: what is switched on; out: False = a null audio pointer
  D1, N1    the prefilter; np1: N1 padded to 8 / 4.  D2, N2, np2: the channel pair.  D = D1 D2: input samples per output
  nout      outputs of the first and the third call (the second has SHORT = 2); part F: of the one call
  cls       CPW by nout alone; cpw, nw, opl: after the fit; al: the second stage's read width; lds: the workgroup's dynamic LDS by the rule
  tile      opl * 64 / cpw; chunks: stage-1 chunks per tile; last: intermediates of the last chunk
  channels  cpw * nw + 1, at most 17: one full workgroup and one with a single valid channel group
  lowered   cpw < cls;  at_cap: lds == 65 536;  refuse: part D, the value one step beyond the limit (a tap count or a factor)

`data(e)` gives the entry's channels (modes, channel taps, oscillator steps and phases), the prefilter row and the input stream, seeded by the
SHAPE alone, so that twins of one shape share their references."""
import functools

import numpy as np

import orclib
import prefilter_model as pm
from decim_census_cases import FIXED_STEPS, _row, _seeded_taps

AM, LSB, USB, CW = orclib.AM, orclib.LSB, orclib.USB, orclib.CW
ARITH = ("q15", "f32")
QUANT = (8, 4)                                     # taps per step: np1 and np2 are multiples of it
MAX_D = (60, 59)                                   # MSDR_MAX_DECIMATION_Q15 / _F32: msdr_chain_set_decimation's own range
TAP_CAP = 4096                                     # msdr_chain_create: num_taps 1 .. 4096
FACTORS = pm.FACTORS
LENGTHS = {4: 30, 2: 130, 1: 258}                  # outputs per call by CPW class: no multiple of any tile
SHORT = 2
MAX_CHANNELS = 17
WORK_CAP = 2 * 10 ** 8                             # multiply-adds of oracle work per entry
CUS = 256
NP1_GRID = tuple(4 ** j for j in range(7))         # x q
SUBSETS = tuple((bool(m & 1), bool(m & 2), bool(m & 4)) for m in range(1, 8))          # (meter, iq, gain)
GAINS = (0.25, 3.0, -2.5, 1.5, 0.7, 12.0, 1.0, -0.4)
C_FACTORS = (2, 16, 32)
C_TAPS = ((2, 4, 6, 8, 10, 16, 30, 34), (1, 2, 3, 4, 5, 7, 8, 33))
C_STAGE2 = (24, 3)                                 # (N2, D2)
C_WHOLE, C_STEP = (32, 32), (8, 4)                 # N2 at D1 = 16: the window a whole number of chunks / a last chunk of one step
D_DECIMATION = ((16, 4, 104), (64, 32, 104))       # (N1, D1, N2)
E_ROW = np.array([30000, -30000] * 7 + [30000, -12000], np.int16)          # sum |p| = 462 000: |acc| reaches 1.5e10 >> 2^31; sum p = 18 000: a constant row passes
E_STAGE2 = (32, 2)                                 # (N2, D2)


def kernel_name(f32, full):
    return "chain_%spcn2_%skernel" % (ARITH[f32], "full_" if full else "")


def stem(f32):
    """what chain.info() names, for the plain body and the twin alike"""
    return "chain_%spcn2_kernel" % ARITH[f32]


def al_of(f32, D2):
    """launch_chain_q15pcn2 / launch_chain_f32pcn2: the widest aligned LDS read of the second stage"""
    if f32:
        return 4 if D2 % 4 == 0 else 2 if D2 % 2 == 0 else 1
    return 0 if D2 & 1 else 4 if D2 % 8 == 0 else 2 if D2 % 4 == 0 else 1


def cls_of(nout):
    return 4 if nout <= 128 else 2 if nout <= 256 else 1


def padded(f32, nt):
    return pm.pad(nt, bool(f32))


def chain_of(cls):
    """the (cpw, nw, opl) the fit walks through, in its order"""
    out = [(cls, 4, 8), (cls, 4, 4), (cls, 4, 2), (cls, 2, 2), (cls, 1, 2)]
    c = cls // 2
    while c >= 1:
        out.append((c, 1, 2))
        c //= 2
    return out


def _lds_grid(f32, np1, D1, np2, D2, cpw, nw, opl):
    """pm.lds_bytes over arrays of np2 and D2"""
    tile = opl * (64 // cpw)
    raw = 2 * (pm.chunk(D1, cpw) * D1 + np1)
    if f32:
        per = 4 * (2 * (tile * D2 + np2) + 2 * np2 + raw)
    else:
        per = 2 * (2 * np.where(D2 & 1, 2, 1) * (tile * D2 + np2) + 2 * np2 + raw)
    return per * cpw * nw + 4096 + np1 * (4 if f32 else 2)


def total_outputs(nout, calls=3):
    return 2 * nout + SHORT if calls == 3 else nout


def work_of(ch, n_in, D1, np1, np2):
    """the oracle's multiply-adds per stream: stage 1 at the full rate, stage 2 at fs / D1"""
    return ch * n_in * np1 + ch * (n_in // D1) * np2


def covered(n_in, D1, np1, np2):
    """the stream is at least as long as both filters: every tap meets a sample"""
    return n_in >= np1 and n_in // D1 >= np2


def reachable():
    """key -> {D1: (work, D1, np1, np2, D2, nout)}: the cheapest covered shape of every reachable key behind every D1"""
    best = {}
    for f32 in (0, 1):
        q = QUANT[f32]
        D2 = np.arange(1, MAX_D[f32] + 1)[:, None]
        np2 = np.arange(q, TAP_CAP + 1, q)[None, :]
        als = [al_of(f32, int(d)) for d in D2[:, 0]]
        for cls, nout in LENGTHS.items():
            outs = total_outputs(nout)
            for D1 in FACTORS:
                n_in = outs * D1 * D2
                for m in NP1_GRID:
                    np1 = q * m
                    idx = np.full((D2.size, np2.size), -1)
                    for k, (cpw, nw, opl) in reversed(list(enumerate(chain_of(cls)))):
                        idx = np.where(_lds_grid(f32, np1, D1, np2, D2, cpw, nw, opl) <= pm.CAP, k, idx)
                    if not (idx >= 0).any():
                        break
                    ok = (n_in >= np1) & (n_in // D1 >= np2)
                    for k, (cpw, nw, opl) in enumerate(chain_of(cls)):
                        ch = min(MAX_CHANNELS, cpw * nw + 1)
                        hit = (idx == k) & ok
                        rows = np.flatnonzero(hit.any(axis=1))
                        first = hit.argmax(axis=1)          # the work grows with np2: the first hit of a row is its cheapest
                        for r in rows:
                            d2, n2 = int(D2[r, 0]), int(np2[0, first[r]])
                            cand = (work_of(ch, outs * D1 * d2, D1, np1, n2), D1, np1, n2, d2, nout)
                            slot = best.setdefault((f32, cls, cpw, nw, opl, als[r]), {})
                            if cand < slot.get(D1, (1 << 62,)):
                                slot[D1] = cand
    return best


def _entry(part, name, f32, D1, N1, D2, N2, nout, meter=False, iq=False, gain=False, agc=False, out=True, calls=3, **more):
    np1, np2 = padded(f32, N1), padded(f32, N2)
    g = pm.geometry(bool(f32), np1, D1, np2, D2, nout, 1, CUS)
    cpw, nw, opl = g["cpw"], g["nw"], g["opl"]
    ch = min(MAX_CHANNELS, cpw * nw + 1)
    g = pm.geometry(bool(f32), np1, D1, np2, D2, nout, ch, CUS)
    wlen, C = g["tile"] * D2 + np2, pm.chunk(D1, cpw)
    e = dict(name=name, part=part, f32=f32, full=meter or iq or gain, meter=meter, iq=iq, gain=gain, agc=agc, out=out, D1=D1, N1=N1, np1=np1, D2=D2, N2=N2,
             np2=np2, D=D1 * D2, nout=nout, cls=cls_of(nout), cpw=cpw, nw=nw, opl=opl, al=al_of(f32, D2), lds=g["lds_bytes"], tile=g["tile"],
             chunks=g["chunks"], last=wlen - (g["chunks"] - 1) * C, channels=ch, lowered=cpw < cls_of(nout), at_cap=g["lds_bytes"] == pm.CAP, refuse=None,
             calls=calls, nseg=g["nseg"])
    assert e["lds"] == pm.lds_bytes(bool(f32), np1, D1, np2, D2, cpw, nw, opl) and e["tile"] == opl * (64 // cpw) and 0 < e["last"] <= C
    assert not agc or gain
    e.update(more)
    return e


def key(e):
    return (e["f32"], e["cls"], e["cpw"], e["nw"], e["opl"], e["al"])


def call_outputs(e):
    return (e["nout"], SHORT, e["nout"]) if e["calls"] == 3 else (e["nout"],)


def total(e):
    """input samples of the whole stream"""
    return sum(call_outputs(e)) * e["D"]


def work(e):
    return work_of(e["channels"], total(e), e["D1"], e["np1"], e["np2"])


def is_covered(e):
    return covered(total(e), e["D1"], e["np1"], e["np2"])


def _limit_shapes(f32):
    """part D, N1 = pre_max_taps: two (D1, N2, D2) whose stream covers the row inside the oracle's budget, one at exactly 64 KB if there is one.
    fp32: a stream of twice the row, so that the row's oldest step weighs more than 1e-4 of the output (tests/test_pre_census_cases.py)"""
    q, nout, found = QUANT[f32], LENGTHS[2], []
    for D1 in FACTORS:
        for D2 in range(1, 25):
            for np2 in range(q, 513, q):
                zero = pm.lds_bytes(bool(f32), 0, D1, np2, D2, 1, 1, 2)
                np1 = (pm.CAP - zero) // (pm.lds_bytes(bool(f32), q, D1, np2, D2, 1, 1, 2) - zero) * q if zero < pm.CAP else 0          # (linear in np1)
                n_in = total_outputs(nout) * D1 * D2
                if np1 and covered(n_in, D1, np1, np2) and (not f32 or n_in >= 2 * np1) and work_of(2, n_in, D1, np1, np2) <= WORK_CAP:
                    cap = pm.lds_bytes(bool(f32), np1, D1, np2, D2, 1, 1, 2) == pm.CAP
                    found.append((not cap, work_of(2, n_in, D1, np1, np2), D1, np1, np2, D2))
    found.sort()
    first = found[0]
    second = next(s for s in found if s[2] != first[2] and s[2] >= 16)          # ... and one behind a wide stage-1 read
    for _, _, D1, np1, np2, D2 in (first, second):
        assert pm.fits(bool(f32), np1, D1, np2, D2) and not pm.fits(bool(f32), np1 + q, D1, np2, D2)
    return [s[2:] for s in (first, second)]


def _build():
    out = []
    best = reachable()
    # A
    part_a, turn = [], {}
    for k in sorted(best):
        f32, cls, cpw, nw, opl, al = k
        i = turn.get((f32, cpw), 0)
        turn[(f32, cpw)] = i + 1
        order = [FACTORS[(i + j) % len(FACTORS)] for j in range(len(FACTORS))]
        D1 = next((d for d in order if d in best[k] and best[k][d][0] <= WORK_CAP), None)
        if D1 is None:
            D1 = min(best[k], key=lambda d: best[k][d])
        _, _, np1, np2, D2, nout = best[k][D1]
        e = _entry("A", "A-%s-c%d-cpw%d-w%d-o%d-al%d-D%d-np%d-D%d-np%d" % (ARITH[f32], cls, cpw, nw, opl, al, D1, np1, D2, np2), f32, D1, np1, D2, np2, nout)
        assert key(e) == k, (k, e)
        part_a.append(e)
    out += part_a
    cost = lambda e: (work(e), e["name"])          # noqa: E731
    # B
    for f32 in (0, 1):
        mine = [e for e in part_a if e["f32"] == f32]
        tag = lambda m, i, g, a=False: "".join(t for t, on in (("m", m), ("q", i), ("g", g), ("a", a)) if on)          # noqa: E731
        iq_only = True
        for n, (cpw, al) in enumerate(sorted({(e["cpw"], e["al"]) for e in mine})):
            a = min((e for e in mine if (e["cpw"], e["al"]) == (cpw, al)), key=cost)
            meter, iq, gain = SUBSETS[n % 7]
            null_out = iq_only and iq and not meter and not gain
            iq_only = iq_only and not null_out
            out.append(_entry("B", "B-%s-%s%s-cpw%d-al%d-D%d-np%d-D%d-np%d" % (ARITH[f32], tag(meter, iq, gain), "-iqonly" if null_out else "", cpw, al, a["D1"], a["np1"],
                                                                              a["D2"], a["np2"]), f32, a["D1"], a["N1"], a["D2"], a["N2"], a["nout"], meter, iq, gain, out=not null_out))
        a = min((e for e in mine if e["lowered"]), key=cost)
        out.append(_entry("B", "B-%s-mqg-lowered-c%d-cpw%d-al%d-D%d-np%d-D%d-np%d" % (ARITH[f32], a["cls"], a["cpw"], a["al"], a["D1"], a["np1"], a["D2"], a["np2"]), f32,
                          a["D1"], a["N1"], a["D2"], a["N2"], a["nout"], True, True, True))
        a = min((e for e in mine if e["cls"] == 2 and not e["lowered"]), key=cost)
        out.append(_entry("B", "B-%s-mqga-agc-cpw%d-al%d-D%d-np%d-D%d-np%d" % (ARITH[f32], a["cpw"], a["al"], a["D1"], a["np1"], a["D2"], a["np2"]), f32,
                          a["D1"], a["N1"], a["D2"], a["N2"], a["nout"], True, True, True, agc=True))
    # C
    for f32 in (0, 1):
        N2, D2 = C_STAGE2
        for D1 in C_FACTORS:
            for N1 in C_TAPS[f32]:
                out.append(_entry("C", "C-%s-D%d-nt%d" % (ARITH[f32], D1, N1), f32, D1, N1, D2, N2, LENGTHS[2]))
        out.append(_entry("C", "C-%s-D16-nt16-whole-chunks" % ARITH[f32], f32, 16, 16, D2, C_WHOLE[f32], LENGTHS[2]))
        out.append(_entry("C", "C-%s-D16-nt16-last-chunk-one-step" % ARITH[f32], f32, 16, 16, D2, C_STEP[f32], LENGTHS[2]))
    # D
    for f32 in (0, 1):
        q = QUANT[f32]
        for D1, np1, np2, D2 in _limit_shapes(f32):
            e = _entry("D", "D-%s-taps-D%d-nt%d-D%d-np%d" % (ARITH[f32], D1, np1, D2, np2), f32, D1, np1, D2, np2, LENGTHS[2], refuse=np1 + q, limit="taps")
            out.append(e)
        for N1, D1, N2 in D_DECIMATION:
            np1, np2, D2 = padded(f32, N1), padded(f32, N2), 0
            while pm.fits(bool(f32), np1, D1, np2, D2 + 1) and D2 < MAX_D[f32]:
                D2 += 1
            e = _entry("D", "D-%s-factor-D%d-nt%d-D%d-np%d" % (ARITH[f32], D1, N1, D2, np2), f32, D1, N1, D2, N2, LENGTHS[2], refuse=D2 + 1, limit="factor")
            out.append(e)
    for e in out:
        if e["part"] == "D" and e["at_cap"]:
            e["name"] += "-lds65536"
    # E
    for D1 in FACTORS:
        out.append(_entry("E", "E-q15-saturate-wrap-D%d" % D1, 0, D1, E_ROW.size, E_STAGE2[1], E_STAGE2[0], LENGTHS[2], iq=True, kind="sat"))
    # F
    for f32 in (0, 1):
        mine = [e for e in part_a if e["f32"] == f32 and e["cls"] == 1 and e["cpw"] == 1 and e["nw"] == 4]
        used = set()
        for opl in (2, 4, 8):
            pool = [e for e in mine if e["opl"] == opl]
            a = min(pool, key=lambda e: (e["al"] in used, work(e) * (8 * e["tile"] + 2), e["name"]))          # spread AL, then the cheapest
            used.add(a["al"])
            e = _entry("F", "F-%s-o%d-al%d-D%d-np%d-D%d-np%d" % (ARITH[f32], opl, a["al"], a["D1"], a["np1"], a["D2"], a["np2"]), f32, a["D1"], a["N1"], a["D2"], a["N2"],
                       8 * a["tile"] + 2, calls=1)
            assert (e["cpw"], e["nw"], e["opl"], e["tile"]) == (1, 4, opl, a["tile"]) and e["nseg"] == 2
            out.append(e)
    for e in out:
        e.setdefault("kind", "")
        e.setdefault("limit", None)
    return out


ENTRIES = _build()
NAMES = [e["name"] for e in ENTRIES]
BY_NAME = {e["name"]: e for e in ENTRIES}


def names(f32):
    return [e["name"] for e in ENTRIES if e["f32"] == f32]


def instantiation(e):
    """(arithmetic, full, CPW, AL) of the kernel the entry's launch selects"""
    return (e["f32"], e["full"], e["cpw"], e["al"])


# ---- the entry's run ------------------------------------------------------------------------------------------------------------------------
def call_slices(e):
    """per call the slice of its outputs in the concatenated output"""
    out, lo = [], 0
    for m in call_outputs(e):
        out.append(slice(lo, lo + m))
        lo += m
    return out


def shape_of(e):
    return (e["f32"], e["D1"], e["N1"], e["D2"], e["N2"], e["nout"], e["calls"], e["channels"], e["kind"])


def _pre_row(f32, rng, D1, nt, n_first):
    """the prefilter row in CMSIS order.  16 taps and more: a windowed-sinc low-pass for decimation by D1 (unit DC gain) of at most the first
    call's length at the NEWEST end, plus a seeded non-zero ripple of 1 .. 60 Q15 units on EVERY coefficient (decim_census_cases._row's
    reasons: the designed edge coefficients are next to nothing, and a row longer than the first call would meet its own tail alone);
    shorter rows: seeded coefficients of magnitude 1000 .. 4000"""
    if nt < 16:
        return _seeded_taps(f32, rng, nt, 1000, 4000)
    m = min(nt, n_first) & ~1
    row = _seeded_taps(0, rng, nt, 1, 60)
    row[nt - m:] += pm.lowpass(D1, m, np.int16)
    return (row.astype(np.float64) / 32768.0).astype(np.float32) if f32 else row


def _sat_rows(rng, ch, n):
    """part E: constant, alternating, random-sign full-scale rows and a random one, in turn"""
    kinds = [np.full(n, 32767, np.int16), np.where(np.arange(n) & 1, -32768, 32767).astype(np.int16)]
    rows = []
    for c in range(ch):
        rows.append(kinds[c % 4] if c % 4 < 2 else rng.choice(np.array([-32768, 32767], np.int16), n) if c % 4 == 2 else rng.integers(-32768, 32768, n).astype(np.int16))
    return np.stack(rows)


@functools.lru_cache(maxsize=None)
def _data(shape):
    f32, D1, N1, D2, N2, nout, calls, ch, kind = shape
    rng = np.random.default_rng([81, f32, D1, N1, D2, N2, nout, calls, ch, len(kind)])
    n = total_outputs(nout, calls) * D1 * D2
    modes = np.array([(AM, LSB, USB, CW)[c % 4] for c in range(ch)], np.int32)
    ti = np.stack([_row(f32, rng, 500.0 + 350.0 * c, N2, nout * D2) for c in range(ch)])
    tq = np.stack([ti[c] if modes[c] == AM else _row(f32, rng, 650.0 + 350.0 * c, N2, nout * D2) for c in range(ch)])
    if kind == "sat":
        steps, phases = np.zeros(ch, np.uint64), np.zeros(ch, np.uint64)          # cos = 32767, sin = 0: the mixer passes the row at 32767 / 32768
        p, x = E_ROW.copy(), _sat_rows(rng, ch, n)
    else:
        steps = np.concatenate([np.array(FIXED_STEPS[:ch], np.uint64), rng.integers(0, 1 << 32, max(0, ch - len(FIXED_STEPS)), dtype=np.uint64)])
        phases = rng.integers(0, 1 << 32, ch, dtype=np.uint64)
        phases[0] = 0x20000000          # the oscillator at step 0 stands still: at 45 degrees both streams carry the input
        p = _pre_row(f32, rng, D1, N1, nout * D1 * D2)
        amp = 20000 if f32 else 30000
        x = rng.integers(-amp, amp + 1, (ch, n)).astype(np.int16)
    gains = np.array([GAINS[c % len(GAINS)] for c in range(ch)], np.float32)
    for a in (steps, phases, modes, ti, tq, p, x, gains):
        a.setflags(write=False)
    return dict(steps=steps, phases=phases, modes=modes, ti=ti, tq=tq, p=p, x=x, n=n, gains=gains)


def data(e):
    return _data(shape_of(e))
