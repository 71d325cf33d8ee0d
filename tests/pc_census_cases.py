"""The census of the sliding-window per-receiver chain kernels -- the kernels a bank runs at D = 1 (minimal-sdr_amd/csrc/msdr_chain_q15pc.hiph,
msdr_chain_f32pc.hiph, msdr_chain_oscpc.hiph, msdr_chain_ncopc.hiph): chain_q15pc / f32pc (with their FIR-only and Fs/4 flavours), chain_q15pco /
f32pco, chain_q15pcn / f32pcn and the metered, I/Q and I/Q-plus-meter twins, 20 templates x 3 channels-per-wave values = 60 instantiations of
pc_frame / pf_frame -- under every launch geometry pc_geometry (msdr_pc_geometry.h) can hand them.

The table is BUILT FROM THE RULE as tests/test_pc_geometry.py restates it (fit, lds_bytes), not written by hand, and holds no GPU code:
tests/test_gpu_pc_census.py (Q15) and tests/test_gpu_pc_census_f32.py run one case per entry, tests/test_pc_census_cases.py checks the table on
the CPU.  A FAMILY is one launcher branch (FAMS below); the Q15 chain with PcOscShared is one instantiation with a run-time branch between Fs/4
and the table in global memory, and has both mixers as two rows.  Six parts:

  A  geometry census, plain kernel.  One entry per reachable key (family, CPW class of n, CPW after the fit, waves): among all padded tap counts
     the setters accept -- multiples of 8 / 4 up to the family's limit, capped at 4096 -- the shortest filter (the cheapest shape).  Call
     lengths 29 / 131 / 259 for the classes 4 / 2 / 1: odd, so that the rows of odd channels start at odd element offsets (the unaligned load
     and store paths run beside the aligned ones), and no multiple of any tile (128 / 256 / 512): every entry ends in a partial tile.  The
     families with a table in global memory also get, per CPW, their cheapest shape with a table of 24 entries (no power of two).
  B  twins.  For each of the 11 twin templates and each CPW: the cheapest part-A shape of that CPW; per twin one entry at its cheapest shape with
     fewer than four waves and one at its cheapest shape whose CPW the fit lowered; per chain family one entry with an input map (two antenna
     rows, the channels alternating between them) at its cheapest shape with fewer than four waves.
  C  tap counts at 131 samples: num_taps exact and padded by every remainder, the one-tap filter (fp32), step counts of all residues mod 3 (fp32).
  D  limits: the longest filter each family's setter accepts (capped at the interface's 4096; beside a row of 128 entries and beside the
     longest row that still leaves a filter, for the row families), processed at 131 samples; `refuse` is the next padded length up.
  E  time segments beside fewer than four waves: per chain family and for 2 and 1 waves, calls of 4600 samples (9 tiles of 512: two segments
     by the rule; the fp32 entries also in the three that time_segments = 3 asks for), plain kernel, metered twin and, where there is one, the
     I/Q twin.
  F  full histories.  The three calls of a part-A entry are 60 / 264 / 520 samples from the zero state: under a filter longer than that the OLDER
     coefficients meet nothing but zeros, and every geometry with fewer than four waves has such a filter (a mutant that stages the oldest 8 / 4
     taps as zeros above 800 taps failed in part E alone).  So every part-A shape whose filter is longer than its stream runs once more behind
     a call of np + 1 samples (odd; one channel per wave) that fills the history: the entry's geometry then works on a window whose every
     sample is alive, and every coefficient moves the output.

An entry (a dict):
  name      unique; the pytest id
  part      "A" .. "F"
  fam       the family's name (FAMS); f32: 0 Q15, 1 fp32; chain: whether it is a chain (the two FIR stages are msdr_fir_* instances)
  mixer     "fs4" / "tab" (one table, global memory) / "rows" (a table row per channel) / "nco" (phase accumulator) / "" (FIR stage)
  osc       entries of the oscillator table (0 where there is none)
  twin      "" / "_meter" / "_iq" / "_iq_meter"
  nt, np    num_taps, and nt padded to 8 / 4
  n         samples of the first and the third call (the second has SHORT = 2)
  cls       CPW by n alone; cpw, nw: after the fit; lds: the workgroup's dynamic LDS by the rule; tile = 512 / cpw
  channels  cpw * nw + 1, at most 17: one full workgroup and one with a single valid channel group and idle waves
  lowered   cpw < cls;  at_cap: lds == 65 536 exactly
  refuse    part D: the num_taps one step beyond the limit (None: the FIR stages, whose own limits lie beyond 4096 taps)
  inmap     msdr_chain_set_input_rows: two antenna rows, channel c hears row c % 2
  warm      part F: samples of the call in front of the three (0 elsewhere)
  ts, nseg  time_segments of the configuration, and the segments the rule then gives the first and the third call on a GPU of 256 CUs

`data(e)` gives the entry's channels (modes, taps, oscillators) and its input stream, seeded by the SHAPE alone, so that twins of one shape share
their references."""
import functools

import numpy as np

import orclib
from decim_census_cases import C_TAPS, FIXED_STEPS, MAX_CHANNELS, QUANT, TAP_CAP, WORK_CAP, _row, bw_taps, padded  # noqa: F401
from gpuhelp import msdr
from test_pc_geometry import CAP, fit, geometry, lds_bytes

AM, LSB, USB, CW = orclib.AM, orclib.LSB, orclib.USB, orclib.CW
LENGTHS = {4: 29, 2: 131, 1: 259}                  # samples per call by CPW class
SHORT = 2                                          # samples of the second call: shorter than every history above 3 taps
LONG = 4600                                        # part E: 9 tiles of 512
CUS = 256                                          # the GPU the expected segment counts are computed for (any GPU gives the same at these channel counts)
ROW_LEN = 128                                      # osc_len of the row families and of the global-table rows
ODD_LEN = 24                                       # a table whose length is no power of two
TWINS = ("", "_meter", "_iq", "_iq_meter")
MIXERS = ("", "fs4", "tab", "rows", "nco")
F32_C_TAPS = C_TAPS[1] + (11,)                     # 11 -> 12 taps = 3 steps: with 1 / 2 / 26 steps of the others all three residues mod 3

# name, arithmetic, the family's name in tests/test_pc_geometry.py, the family whose LDS the SETTER's limit is computed with, kernel stem, the
# rows of the table (mixers), twins, chain or FIR stage
FAMS = (
    dict(name="q15pc", f32=0, geo="q15pc", limit="q15pc", stem="chain_q15pc", mixers=("fs4", "tab"), twins=TWINS[:2], chain=True),
    dict(name="q15fir", f32=0, geo="q15fir", limit=None, stem="chain_q15pc", mixers=("",), twins=TWINS[:1], chain=False),
    dict(name="f32pc", f32=1, geo="f32pc", limit="f32pc", stem="chain_f32pc", mixers=("tab",), twins=TWINS[:2], chain=True),
    dict(name="f32fs4", f32=1, geo="f32fs4", limit="f32pc", stem="chain_f32pc", mixers=("fs4",), twins=TWINS[:2], chain=True),
    dict(name="f32fir", f32=1, geo="f32fir", limit=None, stem="chain_f32pc", mixers=("",), twins=TWINS[:1], chain=False),
    dict(name="q15pco", f32=0, geo="q15pco", limit="q15pco", stem="chain_q15pco", mixers=("rows",), twins=TWINS[:2], chain=True),
    dict(name="f32pco", f32=1, geo="f32pco", limit="f32pco", stem="chain_f32pco", mixers=("rows",), twins=TWINS[:2], chain=True),
    dict(name="q15pcn", f32=0, geo="q15pcn", limit="q15pcn", stem="chain_q15pcn", mixers=("nco",), twins=TWINS, chain=True),
    dict(name="f32pcn", f32=1, geo="f32pcn", limit="f32pcn", stem="chain_f32pcn", mixers=("nco",), twins=TWINS, chain=True),
)
FAM = {f["name"]: f for f in FAMS}
FAM_NAMES = [f["name"] for f in FAMS]


def kernel_name(fam, twin):
    return "%s%s_kernel" % (FAM[fam]["stem"], twin)


def template_of(fam, twin):
    """(kernel, the template arguments behind CPW) as the launchers spell the instantiation"""
    args = {("q15pc", ""): ", false", ("q15fir", ""): ", true", ("f32pc", ""): ", false, false", ("f32fs4", ""): ", false, true",
            ("f32fir", ""): ", true, false", ("f32pc", "_meter"): ", false", ("f32fs4", "_meter"): ", true"}
    return kernel_name(fam, twin), args.get((fam, twin), "")


def cls_of(n):
    return 4 if n <= 128 else 2 if n <= 256 else 1


def osc_of(fam, mixer, osc=None):
    """the table length a row of the table runs with; in the LDS formula only the row families' counts"""
    return 0 if mixer in ("", "fs4", "nco") else (ROW_LEN if osc is None else osc)


def lds_osc(fam, osc):
    return osc if FAM[fam]["geo"] in ("q15pco", "f32pco") else 0


def limit_of(fam, osc=0):
    """the longest padded filter the family's setter accepts, capped at the interface's 4096: one wave with one channel must fit the LDS (the
    chains' limit is that of the general flavour: a chain may change its mixer tables, not its kind); the FIR stages hold longer filters"""
    f = FAM[fam]
    q = QUANT[f["f32"]]
    if f["limit"] is None:
        return TAP_CAP
    np_ = 0
    while np_ + q <= TAP_CAP and lds_bytes(f["limit"], np_ + q, lds_osc(fam, osc), 1, 1) <= CAP:
        np_ += q
    return np_


def longest_row(fam):
    """the longest oscillator row beside which the family's setter still accepts a filter (8 / 4 taps)"""
    f = FAM[fam]
    top = 16384 if not f["f32"] else 8192          # pco_max_taps / f32pco_max_taps refuse longer rows outright
    o = top
    while lds_bytes(f["limit"], QUANT[f["f32"]], o, 1, 1) > CAP:
        o -= 1
    return o


def key_of(fam, np_, n, osc=0):
    """(family, CPW class, CPW, waves) of a launch, None where the rule refuses it"""
    g = fit(FAM[fam]["geo"], n, np_, lds_osc(fam, osc))
    return None if g is None else (fam, cls_of(n), g[0], g[1])


def reachable(lengths):
    """key -> (n * np, np, n) of the cheapest shape, over every filter length the setter accepts"""
    best = {}
    for f in FAMS:
        fam, q = f["name"], QUANT[f["f32"]]
        osc = ROW_LEN if f["mixers"] == ("rows",) else 0
        for np_ in range(q, limit_of(fam, osc) + 1, q):
            for n in lengths:
                k = key_of(fam, np_, n, osc)
                cand = (n * np_, np_, n)
                if k is not None and cand < best.get(k, (1 << 62,)):
                    best[k] = cand
    return best


def _entry(part, name, fam, mixer, twin, nt, n, osc=None, **more):
    f = FAM[fam]
    np_ = padded(f["f32"], nt)
    osc = osc_of(fam, mixer, osc)
    cpw, nw, lds = fit(f["geo"], n, np_, lds_osc(fam, osc))
    ch = min(MAX_CHANNELS, cpw * nw + 1)
    e = dict(name=name, part=part, fam=fam, f32=f["f32"], chain=f["chain"], mixer=mixer, osc=osc, twin=twin, nt=nt, np=np_, n=n, cls=cls_of(n), cpw=cpw,
             nw=nw, lds=lds, tile=512 // cpw, channels=ch, lowered=cpw < cls_of(n), at_cap=lds == CAP, refuse=None, inmap=False, ts=0, warm=0)
    e.update(more)
    e["nseg"] = geometry(f["geo"], n, np_, lds_osc(fam, osc), ch, CUS, e["ts"])[4]
    assert mixer in f["mixers"] and twin in f["twins"]
    return e


def key(e):
    return (e["fam"], e["cls"], e["cpw"], e["nw"])


def tag(e_or_fam, mixer=None):
    fam, mixer = (e_or_fam["fam"], e_or_fam["mixer"]) if mixer is None else (e_or_fam, mixer)
    return fam + ("-" + mixer if len(FAM[fam]["mixers"]) > 1 else "")


def work(e):
    """the oracle's multiply-adds per FIR: channels x total input samples x np"""
    return e["channels"] * total(e) * e["np"]


def _build():
    out = []
    best = reachable(tuple(LENGTHS.values()))
    cost = lambda e: (e["n"] * e["np"], e["name"])          # noqa: E731
    # A
    part_a = []
    for k in sorted(best, key=lambda k: (FAM_NAMES.index(k[0]),) + k[1:]):
        fam, cls, cpw, nw = k
        _, np_, n = best[k]
        for mixer in FAM[fam]["mixers"]:
            part_a.append(_entry("A", "A-%s-c%d-cpw%d-w%d-np%d" % (tag(fam, mixer), cls, cpw, nw, np_), fam, mixer, "", np_, n))
            assert key(part_a[-1]) == k
    for fam in ("q15pc", "f32pc"):
        for cpw in (4, 2, 1):
            a = min((e for e in part_a if e["fam"] == fam and e["mixer"] == "tab" and e["cpw"] == cpw), key=cost)
            part_a.append(_entry("A", "A-%s-osc%d-cpw%d-np%d" % (tag(fam, "tab"), ODD_LEN, cpw, a["np"]), fam, "tab", "", a["nt"], a["n"], osc=ODD_LEN))
    out += part_a
    # B
    for f in FAMS:
        fam, mixer = f["name"], f["mixers"][-1]
        mine = [e for e in part_a if e["fam"] == fam and e["mixer"] == mixer and e["osc"] in (0, ROW_LEN)]
        few = min((e for e in mine if e["nw"] < 4), key=cost)
        low = min((e for e in mine if e["lowered"]), key=cost)
        for twin in f["twins"][1:]:
            for cpw in (4, 2, 1):
                a = min((e for e in mine if e["cpw"] == cpw), key=cost)
                out.append(_entry("B", "B-%s%s-cpw%d-np%d" % (fam, twin, cpw, a["np"]), fam, mixer, twin, a["nt"], a["n"]))
            out.append(_entry("B", "B-%s%s-few-c%d-cpw%d-w%d-np%d" % (fam, twin, few["cls"], few["cpw"], few["nw"], few["np"]), fam, mixer, twin, few["nt"], few["n"]))
            out.append(_entry("B", "B-%s%s-lowered-c%d-cpw%d-w%d-np%d" % (fam, twin, low["cls"], low["cpw"], low["nw"], low["np"]), fam, mixer, twin, low["nt"], low["n"]))
        if f["chain"]:
            out.append(_entry("B", "B-%s-inmap-c%d-cpw%d-w%d-np%d" % (fam, few["cls"], few["cpw"], few["nw"], few["np"]), fam, mixer, "", few["nt"], few["n"], inmap=True))
    # C
    for f in FAMS:
        for mixer in f["mixers"]:
            for nt in (F32_C_TAPS if f["f32"] else C_TAPS[0]):
                out.append(_entry("C", "C-%s-nt%d" % (tag(f["name"], mixer), nt), f["name"], mixer, "", nt, LENGTHS[2]))
    # D
    for f in FAMS:
        fam, q = f["name"], QUANT[f["f32"]]
        for mixer in f["mixers"]:
            for osc in ((ROW_LEN, longest_row(fam)) if mixer == "rows" else (None,)):
                nt = limit_of(fam, osc or 0)
                e = _entry("D", "D-%s%s-nt%d" % (tag(fam, mixer), "-osc%d" % osc if osc else "", nt), fam, mixer, "", nt, LENGTHS[2], osc=osc,
                           refuse=None if f["limit"] is None else nt + q)
                if e["at_cap"]:
                    e["name"] += "-lds65536"
                out.append(e)
    # E
    for f in FAMS:
        if not f["chain"]:
            continue
        fam, mixer = f["name"], f["mixers"][-1]
        osc = ROW_LEN if mixer == "rows" else 0
        for nw in (2, 1):
            np_ = min(np_ for np_ in range(QUANT[f["f32"]], limit_of(fam, osc) + 1, QUANT[f["f32"]]) if key_of(fam, np_, LONG, osc) == (fam, 1, 1, nw))
            for ts in ((0, 3) if f["f32"] else (0,)):
                for twin in f["twins"][:3]:
                    out.append(_entry("E", "E-%s%s-w%d-np%d-ts%d" % (fam, twin, nw, np_, ts), fam, mixer, twin, np_, LONG, ts=ts))
    # F
    for a in part_a:
        if a["osc"] != ODD_LEN and a["np"] > 2 * a["n"] + SHORT:
            out.append(_entry("F", "F" + a["name"][1:], a["fam"], a["mixer"], "", a["nt"], a["n"], warm=a["np"] + 1))
    return out


ENTRIES = _build()
NAMES = [e["name"] for e in ENTRIES]
BY_NAME = {e["name"]: e for e in ENTRIES}


def names(f32):
    return [e["name"] for e in ENTRIES if e["f32"] == f32]


# ---- the entry's run ------------------------------------------------------------------------------------------------------------------------
def calls(e):
    return ((e["warm"],) if e["warm"] else ()) + (e["n"], SHORT, e["n"])


def read_at(e):
    """the calls behind which chain.info() is read: the two of the entry's length"""
    return (1, 3) if e["warm"] else (0, 2)


def total(e):
    return e["warm"] + 2 * e["n"] + SHORT


def shape_of(e):
    return (e["fam"], e["mixer"], e["osc"], e["nt"], e["n"], e["channels"], e["inmap"], e["warm"])


def osc_rows(ch, L, seed=0):
    """(osc_i, osc_q) int16 [ch, L]: a different bin and a different start phase per channel (rows of tests/test_gpu_osc_per_channel.py)"""
    k = (1 + seed + 3 * np.arange(ch)) % L
    ph = 0.37 * (1 + seed) + 0.61 * np.arange(ch)
    a = 2 * np.pi * k[:, None] * np.arange(L)[None, :] / L + ph[:, None]
    return np.round(32767 * np.sin(a)).astype(np.int16), np.round(32767 * np.cos(a)).astype(np.int16)


def as_f32(v):
    """Q15 oscillator values as the fp32 chains take them (exact)"""
    return (v.astype(np.float64) / 32768.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _data(shape):
    fam, mixer, osc, nt, n, ch, inmap, warm = shape
    f32 = FAM[fam]["f32"]
    rng = np.random.default_rng([78, FAM_NAMES.index(fam), MIXERS.index(mixer), osc, nt, n, ch, int(inmap), warm])
    steps = np.concatenate([np.array(FIXED_STEPS[:ch], np.uint64), rng.integers(0, 1 << 32, max(0, ch - len(FIXED_STEPS)), dtype=np.uint64)])
    phases = rng.integers(0, 1 << 32, ch, dtype=np.uint64)
    phases[0] = np.uint64(0x20000000) | (phases[0] & np.uint64(0x0FFFFFFF))          # channel 0 stands still (step 0): between 45 and 67.5 degrees, I and Q both alive
    modes =np.array([(AM, LSB, USB, CW)[c % 4] for c in range(ch)], np.int32)
    ti = np.stack([_row(f32, rng, 500.0 + 350.0 * c, nt, n) for c in range(ch)])
    tq = np.stack([ti[c] if modes[c] == AM else _row(f32, rng, 650.0 + 350.0 * c, nt, n) for c in range(ch)])
    m = warm + 2 * n + SHORT
    if not FAM[fam]["chain"] and f32:
        x = rng.standard_normal((ch, m)).astype(np.float32)          # arm_fir_f32: float samples
    else:
        amp = 20000 if f32 else 30000
        x = rng.integers(-amp, amp + 1, (ch, m)).astype(np.int16)
    d = dict(steps=steps, phases=phases, modes=modes, ti=ti, tq=tq, x=x, n=m, oi=None, oq=None)
    if mixer in ("tab", "rows"):
        d["oi"], d["oq"] = osc_rows(ch if mixer == "rows" else 1, osc, seed=5)
    for a in d.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return d


def data(e):
    return _data(shape_of(e))


def heard(e):
    """the input row every channel hears: [channels, total]"""
    d = data(e)
    return d["x"][np.arange(e["channels"]) % 2] if e["inmap"] else d["x"]


def oscillator(e, m):
    """(osc_i "sin", osc_q "cos") int16 [channels, m]: the oscillator values the first m samples of the stream meet, channel by channel"""
    d, ch = data(e), e["channels"]
    if e["mixer"] == "fs4":          # Minimal-SDR.ino:546-558 as a table of four entries
        t = np.arange(m) % 4
        return np.tile(np.array([0, 1, 0, -1], np.int16)[t], (ch, 1)), np.tile(np.array([1, 0, -1, 0], np.int16)[t], (ch, 1))
    if e["mixer"] == "nco":
        ph = (d["phases"][:, None] + np.arange(m, dtype=np.uint64)[None, :] * d["steps"][:, None]) & np.uint64(0xFFFFFFFF)
        s, c = msdr.nco_q15(ph.astype(np.uint32))
        return s.reshape(ph.shape), c.reshape(ph.shape)
    pos = np.arange(m) % e["osc"]
    oi, oq = d["oi"][:, pos], d["oq"][:, pos]
    return (oi, oq) if e["mixer"] == "rows" else (np.tile(oi, (ch, 1)), np.tile(oq, (ch, 1)))
