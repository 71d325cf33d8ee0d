"""The census of the gain twins (minimal-sdr_amd/csrc/msdr_chain_gncopc.hip, msdr_chain_gdecpc.hip, msdr_chain_gain.hiph: the code behind
msdr_chain_set_gain): chain_{q15,f32}pcn[_cx]_gain_kernel<CPW> and chain_{q15,f32}pcnd[_cx]_gain_kernel<CPW, AL> -- 8 templates, 12 + 24 + 18 = 54
instantiations, each the superset body (meter, pairs and gain compiled in, p.meter / p.iq switched at run time) under an occupancy attribute
of its own -- and agc_step_kernel behind them, under every launch geometry their plain twins can be handed.

The table is DERIVED from the censuses of the plain kernels and re-derives no geometry: the four gain launchers say that validation, geometry
and LDS are the plain twins' own (tests/test_gain_census_cases.py holds them to that, from their text).  Parents are the entries of
tests/pc_census_cases.py (families q15pcn, f32pcn) and tests/decim_census_cases.py.  It holds no GPU code: tests/test_gpu_gain_census.py (Q15)
and tests/test_gpu_gain_census_f32.py run one case per entry, tests/test_gain_census_cases.py checks the table on the CPU.  Seven parts:

  A  geometry.  Every reachable key of both parents' part A (24 sliding-window, 120 decimating) run by the gain twin with audio, pairs and
     meter on, fixed per-receiver gains (A_GAINS: 1.0, a negative gain, 40, a fraction, and from five receivers on a zero), AGC off.  Inside
     each group (arithmetic, kind, CPW, AL) the input alternates real / complex, and `dir` alternates among the complex entries of a template:
     every one of the 54 instantiations occurs, and every _cx_ template meets both directions.
  B  the superset's switches.  Per instantiation its cheapest part-A shape, {meter, pairs} rotating through the four subsets; where the pairs
     are on and the meter is off every second entry makes I/Q-only calls (a null audio pointer).  AGC on for every receiver: the multiplier
     changes between the three calls.  Per template one entry at its cheapest shape whose CPW the fit lowered, and per sliding-window template
     one with an input map (the parents' inmap shapes).
  C  arithmetic corners, per template and CPW (AL rotating on the decimating ones), at the cheapest part-A shape with five receivers or more.
     Q15: the bank of agc_model.corners() carried to the entry's shape (stream "corners": receivers 0 mod 4 wrap the accumulator under gain
     0.25, 1 mod 4 wrap it in both streams under -2.5 -- with complex input the mixer's sum leaves int16 there --, 2 mod 4 have a zero
     multiplier, 3 mod 4 saturate at both rails under gain 40).  fp32: gains -2.5, 1e6 (clamped to 32767), 40 (the peak over in_scale passes
     32767: absmax clamps), 0, 0.25.
  D  the peak's boundary, per instantiation.  Stream "burst": the receivers 0 mod 4 are AM on a constant oscillator, hear +-40 with the LAST
     THREE input samples at 30 000, through a filter whose three newest coefficients are small and whose older ones are large: the outputs of
     the call meet the burst with the small ones, the outputs past n_out (same tile, never stored) with the large ones.  A kernel that counted
     them would report the peak of the stream followed by zeros to the tile's end: `longer` > 4 `true` > 0 in the model, on every burst receiver.
     The shape is the cheapest of the instantiation whose filter is longer than D + 4 (a shorter one shows the outputs past n_out no burst).
  E  limits.  The parents' part-D entries (the longest filters, those at exactly 65 536 bytes of LDS among them), gain on, alternating real /
     complex.  `refuse` stays the parents' business.
  F  time segments.  The sliding-window parents' part-E shapes of the plain kernel (4600 samples, two and one waves, ts 0, and 3 on fp32) as
     real and as complex input; per arithmetic two decimating shapes for which dec_geometry gives two segments at these channel counts, one
     with four waves and one with fewer (the cheapest by the rule as tests/test_decim_geometry.py restates it).  Each carries the burst.
  G  the step kernel's grid: per arithmetic 65 and 130 receivers at the cheapest sliding-window shape (a second workgroup of one lane; a third
     of two), AGC on for every second receiver.  These entries lift the parents' cap of 17 channels.

An entry is its parent's dict (pc_census_cases / decim_census_cases say what the fields mean; on the decimating entries inmap = False, warm = 0,
ts = 0 and nseg by the rule, as in tests/cx_census_cases.py) with
  name      unique; the pytest id          part      "A" .. "G"          parent    the parent's name
  kind      "pc" (sliding window) / "dec" (decimating)
  cx, dir   complex input and its direction (dir 0 on real entries)
  meter, iq, out     what the calls set: the meter, the I/Q buffer, the audio batch (False = a null audio pointer)
  agc       per receiver 0 / 1          gains     per receiver, float
  stream    "parent" / "corners" / "burst": what data(e) changes in the parent's channels
  unjudged  the receivers the float64 clause (e_orc < 2e-6) cannot judge: those with a zero gain (held to exact zeros instead)

`data(e)` is seeded by the SHAPE alone (the parent's shape and the stream), so entries of one shape share references; it is the cx census's
data -- the parents' streams, taps and oscillators and the Q stream xq -- with the receivers a stream names rewritten.  Calls are the parents'
three: the entry's length, 2, the entry's length again."""
import functools

import numpy as np

import cx_census_cases as cx
import decim_census_cases as dec
import pc_census_cases as pc
from cx_cases import interleave
from test_decim_geometry import fit as dec_fit
from test_decim_geometry import geometry as dec_geometry

PC_FAMS = cx.PC_FAMS
ARITH = dec.ARITH
WORK_CAP = dec.WORK_CAP
CUS = pc.CUS
SEED = 80                                          # (the parents' streams: 77, 78; the cx census's: 79)
AM, LSB, USB = pc.AM, pc.LSB, pc.USB
A_GAINS = (1.0, -2.5, 40.0, 0.25, 0.0, 3.0, 0.7, 12.0)
B_GAINS = (4.0, 1.0, 20.0, 0.5, 2.0, 37.5, 0.7, 12.0)          # where the AGC starts
Q15_CORNERS = (0.25, -2.5, 0.0, 40.0)                           # agc_model.corners()
F32_CORNERS = (-2.5, 1e6, 40.0, 0.0, 0.25)
BURST_GAINS = (1.0, -3.0, 2.0)                                   # the burst receivers (0 mod 4), in turn
BURST_OTHERS = (2.0, 0.5, 12.0)
BURST_EVERY = 4
BURST_LEVEL, QUIET = 30000, 40
BURST_TAPS = (8000, 300)                                         # the older coefficients, the three newest (Q15 units)
SUBSETS = ((False, False), (True, False), (False, True), (True, True))          # (meter, pairs)
G_CHANNELS = (65, 130)


def template_of(f32, kind, is_cx):
    """the __global__ template the entry's launch selects"""
    return "chain_%spcn%s_%sgain_kernel" % (ARITH[f32], "d" if kind == "dec" else "", "cx_" if is_cx else "")


def instantiation(e):
    """(template, CPW, AL) by the launchers' rules: cx, CPW after the fit, al_of(D); AL None for the sliding-window twins"""
    return (template_of(e["f32"], e["kind"], e["cx"]), e["cpw"], dec.al_of(e["f32"], e["D"]) if e["kind"] == "dec" else None)


def mangled(inst):
    """the needle tests/test_agc_pc_kernel.py looks the instantiation up with"""
    t, cpw, al = inst
    return "%sILi%dE%sE" % (t, cpw, "" if al is None else "Li%dE" % al)


def cycle(values, ch):
    return tuple(float(values[c % len(values)]) for c in range(ch))


def _mk(part, tag, kind, p, is_cx, direction, meter=True, iq=True, out=True, agc=0, gains=A_GAINS, stream="parent", **more):
    e = dict(p)
    if kind == "dec":
        e.update(inmap=False, warm=0, ts=0)
    e.update(more)
    ch = e["channels"]
    if kind == "dec":
        e["nseg"] = dec_geometry(e["f32"], e["D"], e["np"], e["nout"], ch, CUS, 0)[4]
    if stream == "burst":
        g = tuple(float(BURST_GAINS[(c // BURST_EVERY) % 3] if c % BURST_EVERY == 0 else BURST_OTHERS[c % 3]) for c in range(ch))
        agc = tuple(int(c % BURST_EVERY == 1) for c in range(ch))          # (a burst receiver's gain stays: the AGC would turn a quiet one up to the rails)
    else:
        g = cycle(gains, ch)
        agc = tuple(int(c & 1) for c in range(ch)) if agc == "odd" else (int(agc),) * ch
    e.update(name="%s-%s-%s%s" % (part, p["name"], "cx%d" % direction if is_cx else "re", tag), part=part, parent=p["name"], kind=kind, cx=bool(is_cx),
             dir=direction if is_cx else 0, meter=meter, iq=iq, out=out, agc=agc, gains=g, stream=stream, twin="",
             unjudged=tuple(c for c in range(ch) if g[c] == 0.0))
    return e


def work(e):
    return cx.work(e)


def _cost(e_or_p_kind):
    kind, p = e_or_p_kind
    return ((pc if kind == "pc" else dec).work(p), p["name"])


def _dec_segmented(f32, few):
    """the cheapest decimating shape (D, np, nout) whose three calls run in two time segments: a tile count of 8 (pc_geometry's rule: tiles / 4
    segments) ending in a partial tile, with four waves or with fewer"""
    best = None
    for D in range(2, dec.MAX_D[f32] + 1):
        for np_ in range(dec.padded(f32, D + 4), min(dec.max_taps(f32, D), 512) + 1, dec.QUANT[f32]):          # (part D's condition on the filter)
            f = dec_fit(f32, np_, D, 1 << 20)
            if f is None or (f[1] < 4) != few:
                continue
            tile = f[2] * (64 // f[0])
            nout = 7 * tile + 3
            cand = (nout * D * np_, D, np_, nout)
            if dec_geometry(f32, D, np_, nout, f[0] * f[1] + 1, CUS, 0)[4] >= 2 and (best is None or cand < best):
                best = cand
    return best[1:]


def _dec_longer_than_factor(f32, cpw, al):
    """the cheapest decimating shape (D, np, nout) of one (CPW, AL) pair whose filter is longer than D + 4"""
    best = None
    for D in range(2, dec.MAX_D[f32] + 1):
        if dec.al_of(f32, D) != al:
            continue
        for np_ in range(dec.padded(f32, D + 4), min(dec.max_taps(f32, D), dec.TAP_CAP) + 1, dec.QUANT[f32]):
            for nout in dec.LENGTHS.values():
                f = dec_fit(f32, np_, D, nout)
                cand = (nout * D * np_, D, np_, nout)
                if f is not None and f[0] == cpw and (best is None or cand < best):
                    best = cand
    return best[1:]


def _build():
    out = []
    dirs = {}

    def turn(f32, kind, is_cx):
        """the direction of the template's next complex entry"""
        if not is_cx:
            return 0
        t = template_of(f32, kind, True)
        dirs[t] = dirs.get(t, -1) + 1
        return dirs[t] % 2

    pa = [("pc", p) for p in pc.ENTRIES if p["part"] == "A" and p["fam"] in PC_FAMS] + [("dec", p) for p in dec.ENTRIES if p["part"] == "A"]
    group = lambda kp: (kp[1]["f32"], kp[0], kp[1]["cpw"], kp[1]["al"] if kp[0] == "dec" else -1)          # noqa: E731
    groups = {}
    for kp in pa:
        groups.setdefault(group(kp), []).append(kp)
    # A
    part_a = []
    for k in sorted(groups):
        members = groups[k]
        for i, (kind, p) in enumerate(members):
            for is_cx in ([i % 2] if len(members) > 1 else [0, 1]):
                part_a.append(_mk("A", "", kind, p, is_cx, turn(p["f32"], kind, is_cx)))
    out += part_a
    # B
    insts = sorted({instantiation(e) for e in part_a}, key=lambda t: (t[0], t[1], -1 if t[2] is None else t[2]))
    iq_only = {}
    for i, inst in enumerate(insts):
        is_cx = "_cx_" in inst[0]
        kind, p = min(((kind, p) for kind, p in pa if instantiation(_mk("B", "", kind, p, is_cx, 0)) == inst), key=_cost)
        meter, iq = SUBSETS[(i + i // 4) % 4]
        audio = True
        if iq and not meter:
            iq_only[(p["f32"], kind)] = iq_only.get((p["f32"], kind), 0) + 1          # (counted per arithmetic and kind: each makes such calls)
            audio = iq_only[(p["f32"], kind)] % 2 == 0
        out.append(_mk("B", "-m%di%da%d" % (meter, iq, audio), kind, p, is_cx, turn(p["f32"], kind, is_cx), meter, iq, audio, agc=1, gains=B_GAINS))
    for f32 in (0, 1):
        for kind in ("pc", "dec"):
            low = min((kp for kp in pa if kp[0] == kind and kp[1]["f32"] == f32 and kp[1]["lowered"]), key=_cost)
            few = [kp for kp in (("pc", p) for p in pc.ENTRIES if p["part"] == "B" and p["inmap"] and p["fam"] in PC_FAMS) if kp[1]["f32"] == f32]
            for is_cx in (0, 1):
                out.append(_mk("B", "-lowered", kind, low[1], is_cx, turn(f32, kind, is_cx), agc=1, gains=B_GAINS))
                if kind == "pc":
                    assert len(few) == 1
                    out.append(_mk("B", "", "pc", few[0][1], is_cx, turn(f32, "pc", is_cx), agc=1, gains=B_GAINS))
    # C
    for f32 in (0, 1):
        for kind in ("pc", "dec"):
            for is_cx in (0, 1):
                for j, cpw in enumerate((4, 2, 1)):
                    mine = [kp for kp in pa if kp[0] == kind and kp[1]["f32"] == f32 and kp[1]["cpw"] == cpw and kp[1]["channels"] >= 5]
                    if kind == "dec":
                        als = sorted({p["al"] for _, p in mine})
                        al = als[(j + is_cx) % len(als)]
                        mine = [kp for kp in mine if kp[1]["al"] == al]
                    kp = min(mine, key=_cost)
                    out.append(_mk("C", "", kind, kp[1], is_cx, turn(f32, kind, is_cx), agc=1, gains=F32_CORNERS if f32 else Q15_CORNERS,
                                   stream="parent" if f32 else "corners"))
    # D
    for inst in insts:
        is_cx = "_cx_" in inst[0]
        mine = [kp for kp in pa if instantiation(_mk("D", "", kp[0], kp[1], is_cx, 0)) == inst and kp[1]["np"] >= kp[1].get("D", 1) + 4]
        if mine:
            kind, p = min(mine, key=_cost)
        else:          # no part-A shape of the instantiation has such a filter: the cheapest shape of the instantiation that has
            f32 = int("f32" in inst[0])
            D, np_, nout = _dec_longer_than_factor(f32, inst[1], inst[2])
            kind, p = "dec", dec._entry("D", "D-%s-cpw%d-al%d-D%d-np%d" % (ARITH[f32], inst[1], inst[2], D, np_), f32, "", D, np_, nout)
        assert instantiation(_mk("D", "", kind, p, is_cx, 0)) == inst
        out.append(_mk("D", "", kind, p, is_cx, turn(p["f32"], kind, is_cx), stream="burst"))
    # E
    limits = [("pc", p) for p in pc.ENTRIES if p["part"] == "D" and p["fam"] in PC_FAMS] + [("dec", p) for p in dec.ENTRIES if p["part"] == "D"]
    for i, (kind, p) in enumerate(limits):
        out.append(_mk("E", "", kind, p, i % 2, turn(p["f32"], kind, i % 2), refuse=None))
    # F
    for p in pc.ENTRIES:
        if p["part"] == "E" and p["fam"] in PC_FAMS and p["twin"] == "":
            for is_cx in (0, 1):
                out.append(_mk("F", "", "pc", p, is_cx, turn(p["f32"], "pc", is_cx), stream="burst"))
    for f32 in (0, 1):
        for few in (False, True):
            D, np_, nout = _dec_segmented(f32, few)
            p = dec._entry("F", "F-%s-D%d-np%d-nout%d" % (ARITH[f32], D, np_, nout), f32, "", D, np_, nout)
            for is_cx in (0, 1):
                out.append(_mk("F", "", "dec", p, is_cx, turn(f32, "dec", is_cx), stream="burst"))
    # G
    for fam in PC_FAMS:
        p = min((kp for kp in pa if kp[0] == "pc" and kp[1]["fam"] == fam), key=_cost)[1]
        for ch in G_CHANNELS:
            out.append(_mk("G", "-ch%d" % ch, "pc", p, 0, 0, agc="odd", channels=ch))
    return out


ENTRIES = _build()
NAMES = [e["name"] for e in ENTRIES]
BY_NAME = {e["name"]: e for e in ENTRIES}


def names(f32):
    return [e["name"] for e in ENTRIES if e["f32"] == f32]


def parent_of(e):
    """the parent's entry (part F's decimating shapes are this table's own: None)"""
    return (pc if e["kind"] == "pc" else dec).BY_NAME.get(e["parent"])


def stem(e):
    """what chain.info() names: the plain kernel's stem (the names stay under msdr_chain_set_gain)"""
    return cx.stem(e)


# ---- the entry's run: the cx census's (calls are OUTPUTS; total and out_index are INPUT samples) ---------------------------------------------
factor, calls, total, out_index, call_slices, heard = cx.factor, cx.calls, cx.total, cx.out_index, cx.call_slices, cx.heard


def pad(e):
    """input samples behind the stream that the last call's partly live tile would cover: the outputs past n_out the peak must not count"""
    return (-calls(e)[-1]) % e["tile"] * factor(e)


def burst_receivers(e):
    return tuple(range(0, e["channels"], BURST_EVERY)) if e["stream"] == "burst" else ()


def burst_taps(f32, nt):
    t = np.full(nt, BURST_TAPS[0], np.int16)
    t[-3:] = BURST_TAPS[1]
    return (t.astype(np.float64) / 32768.0).astype(np.float32) if f32 else t


def shape_of(e):
    return cx.shape_of(e) + (e["stream"],)


@functools.lru_cache(maxsize=None)
def _data(shape):
    base, stream = cx._data(shape[:-1]), shape[-1]
    if stream == "parent":
        return base
    d = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    f32 = pc.FAM[shape[1]]["f32"] if shape[0] == "pc" else shape[1]
    rng = np.random.default_rng([SEED] + cx._seed(shape[:-1])[1:])
    ch, n = d["x"].shape
    nt = d["ti"].shape[1]
    if stream == "burst":
        for c in range(0, ch, BURST_EVERY):
            d["modes"][c], d["steps"][c], d["phases"][c] = AM, 0, 0x20000000          # a constant oscillator: cos = sin = 23170
            d["ti"][c] = d["tq"][c] = burst_taps(f32, nt)
            d["x"][c], d["xq"][c] = rng.integers(-QUIET, QUIET + 1, (2, n))
            d["x"][c, -3:] = BURST_LEVEL
    else:          # "corners" (Q15)
        assert stream == "corners" and not f32
        for c in range(ch):
            if c % 4 < 2:
                d["ti"][c] = d["tq"][c] = 32767
                d["x"][c] = d["xq"][c] = -32768
                d["steps"][c], d["phases"][c] = 0, (0, 0x20000000)[c % 4]
            d["modes"][c] = (AM, LSB, USB, AM)[c % 4]
    d["pairs"] = interleave(d["x"], d["xq"])
    d["pairs_q0"] = interleave(d["x"], np.zeros_like(d["xq"]))
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def data(e):
    """the cx census's data of the entry's shape (modes, taps, steps, phases, x, xq, pairs) with the stream's receivers rewritten"""
    return _data(shape_of(e))
