"""The conditions on the table of the census of the gain twins (tests/gain_census_cases.py), checked without a GPU:

  * all 54 instantiations -- the names as tests/test_agc_pc_kernel.py builds them -- occur in part A, in part B and in part D; the
    instantiation an entry selects is read from the launchers' rules (cx, CPW after the fit, al_of(D), whose expressions are in the text of
    msdr_chain_gdecpc.hip); every _cx_ template meets both directions in part A; names are unique and no entry exceeds the parents' cap of
    oracle work;
  * the geometry is not re-derived because the gain launchers ARE the plain ones: the text of every launch_chain_*_gain is its plain twin's
    with the parameter block's type, the `cx` argument, p.agc and cx_ok() in the validity and the twin chosen by cx in place of the choice by
    p.iq / p.meter -- the same LDS functions, the same read-width expressions; and every entry's geometry equals the parents' rule's;
  * per Q15 entry, from the model and the oracle alone: the expected audio, pairs and meter are alive; part C reaches every named corner
    (a wrapped accumulator under a gain and under a negative gain, a zero multiplier, both rails, on complex entries the mixer's second
    saturation); parts D and F meet the burst rule longer > 4 true > 0 on every burst receiver;
  * per fp32 entry: e_orc < 2e-6 on every judged receiver (the clause that keeps the GPU files' other two honest), the receivers not judged
    are those with a zero gain and at most one in four; part C's gains reach the clamp and the absmax's clamp; the burst rule in D and F."""
import re

import numpy as np
import pytest

import agc_model as M
import decim_census_cases as dec
import gain_census_cases as cases
import pc_census_cases as pc
import test_gpu_gain_census as q15
import test_gpu_gain_census_f32 as fp32
from cx_cases import rel
from f32judge import oracle
from test_agc_pc_kernel import TWINS
from test_cx_census_cases import launchers, source
from test_decim_geometry import fit as dec_fit
from test_decim_geometry import geometry as dec_geometry
from test_pc_geometry import fit as pc_fit
from test_pc_geometry import geometry as pc_geometry

ENTRIES = cases.ENTRIES
COUNTS = dict(A=144, B=54 + 8 + 4, C=24, D=54, E=9, F=12 + 8, G=4)


def part(letter):
    return [e for e in ENTRIES if e["part"] == letter]


def test_the_parts_and_every_instantiation_in_a_b_and_d():
    assert len(set(cases.NAMES)) == len(ENTRIES) == sum(COUNTS.values()) and {k: len(part(k)) for k in COUNTS} == COUNTS
    assert len(TWINS) == 54 == len(set(TWINS))
    for letter in "ABD":
        found = {cases.mangled(cases.instantiation(e)) for e in part(letter)}
        assert found == set(TWINS), (letter, sorted(set(TWINS) - found), sorted(found - set(TWINS)))
    # the rules the instantiation is read with: the read widths' expressions and the choice by cx are in the launchers' text
    body = launchers(source("msdr_chain_gdecpc.hip"))
    assert "(D & 1) ? 0 : (D % 8 == 0) ? 4 : (D % 4 == 0) ? 2 : 1" in body["launch_chain_q15pcnd_gain"][1]
    assert "(D % 4 == 0) ? 4 : (D % 2 == 0) ? 2 : 1" in body["launch_chain_f32pcnd_gain"][1] and "AL = decltype(a)::value == 0 ? 1 : decltype(a)::value" in body["launch_chain_f32pcnd_gain"][1]
    templates = {cases.instantiation(e)[0] for e in part("A")}
    assert len(templates) == 8
    for t in sorted(templates):
        if "_cx_" in t:
            assert {e["dir"] for e in part("A") if cases.instantiation(e)[0] == t} == {0, 1}, t
    for e in ENTRIES:
        assert cases.work(e) <= cases.WORK_CAP == dec.WORK_CAP == pc.WORK_CAP, (e["name"], cases.work(e))
        assert len(e["gains"]) == len(e["agc"]) == e["channels"] and (e["out"] or e["iq"]) and (e["cx"] or e["dir"] == 0), e["name"]
        assert e["channels"] == (min(17, e["cpw"] * e["nw"] + 1) if e["part"] != "G" else e["channels"]) and cases.calls(e)[-1] % e["tile"], e["name"]
    print({k: len(part(k)) for k in COUNTS}, "Q15 %d fp32 %d" % (len(cases.names(0)), len(cases.names(1))))


def test_what_the_parts_promise():
    a, b = part("A"), part("B")
    assert sorted(e["parent"] for e in a if e["kind"] == "pc") == sorted(p["name"] for p in pc.ENTRIES if p["part"] == "A" and p["fam"] in cases.PC_FAMS)
    assert len({e["parent"] for e in a if e["kind"] == "pc"}) == 24 and len({e["parent"] for e in a if e["kind"] == "dec"}) == 120
    assert all(e["meter"] and e["iq"] and e["out"] and not any(e["agc"]) and e["stream"] == "parent" for e in a + part("E"))
    assert all({0.0, -2.5, 40.0, 1.0, 0.25} <= set(e["gains"]) for e in a if e["channels"] >= 5) and any(e["channels"] >= 5 for e in a)
    # B: the four subsets, I/Q-only calls, AGC on everywhere; the lowered entries and the input maps per template
    per = b[:54]
    assert {(e["meter"], e["iq"]) for e in per} == set(cases.SUBSETS) and all(all(e["agc"]) for e in b)
    tapped = [e for e in per if e["iq"] and not e["meter"]]
    for arith in (0, 1):          # every second of them, counted per arithmetic and kind, makes I/Q-only calls
        for kind in ("pc", "dec"):
            mine = [e["out"] for e in tapped if (e["f32"], e["kind"]) == (arith, kind)]
            assert mine and mine == [i % 2 == 1 for i in range(len(mine))], (arith, kind, mine)
    assert all(e["out"] for e in ENTRIES if e not in tapped)
    for arith in (0, 1):          # both arithmetics make I/Q-only calls through a sliding-window and a decimating twin
        assert {e["kind"] for e in per if e["f32"] == arith and not e["out"]} == {"pc", "dec"}
    assert {cases.instantiation(e)[0] for e in b if e["lowered"] and e["name"].endswith("-lowered")} == {cases.instantiation(e)[0] for e in a} and sum(e["name"].endswith("-lowered") for e in b) == 8
    assert sorted(cases.instantiation(e)[0] for e in b if e["inmap"]) == sorted(t for t in {cases.instantiation(e)[0] for e in a} if "pcnd" not in t)
    # C: per template and CPW, every read width among the decimating ones
    c = part("C")
    assert len({cases.instantiation(e)[:2] for e in c}) == 24 and all(e["channels"] >= 5 and all(e["agc"]) for e in c)
    for arith, als in ((0, {0, 1, 2, 4}), (1, {1, 2, 4})):
        assert {e["al"] for e in c if e["kind"] == "dec" and e["f32"] == arith} == als
    # E: the parents' limits, those at the LDS cap among them, both inputs
    lim = part("E")
    assert sorted(e["parent"] for e in lim) == sorted([p["name"] for p in pc.ENTRIES if p["part"] == "D" and p["fam"] in cases.PC_FAMS] + [p["name"] for p in dec.ENTRIES if p["part"] == "D"])
    assert sum(e["at_cap"] for e in lim) >= 2 and {e["cx"] for e in lim} == {False, True} and all(e["refuse"] is None for e in ENTRIES)
    # F: segments beside fewer than four waves, and behind a decimator with four waves and with fewer
    f = part("F")
    assert all(e["nseg"] >= 2 and e["stream"] == "burst" for e in f) and all(e["nseg"] == 1 for e in ENTRIES if e["part"] not in "F")
    assert {(e["f32"], e["nw"], e["ts"]) for e in f if e["kind"] == "pc"} == {(0, 2, 0), (0, 1, 0), (1, 2, 0), (1, 1, 0), (1, 2, 3), (1, 1, 3)}
    for arith in (0, 1):
        waves = {e["nw"] for e in f if e["kind"] == "dec" and e["f32"] == arith}
        assert 4 in waves and min(waves) < 4 and {e["cx"] for e in f if e["kind"] == "dec" and e["f32"] == arith} == {False, True}
    # G: a second workgroup of agc_step_kernel (64 lanes each), a partial last one; AGC on every second receiver
    assert sorted((e["f32"], e["channels"]) for e in part("G")) == [(0, 65), (0, 130), (1, 65), (1, 130)] and all(e["agc"] == tuple(c & 1 for c in range(e["channels"])) for e in part("G"))
    assert "hipLaunchKernelGGL(agc_step_kernel, dim3((c->channels + 63) / 64), dim3(64)," in source("msdr_api.hip")


def test_every_entrys_geometry_is_the_parents_rules():
    for e in ENTRIES:
        p = cases.parent_of(e)
        if p is not None:
            keep = set(p) - {"name", "part", "twin", "refuse", "nseg"} - ({"channels"} if e["part"] == "G" else set())
            assert all(e[k] == p[k] for k in keep), e["name"]
        if e["kind"] == "pc":
            geo = pc.FAM[e["fam"]]["geo"]
            assert pc_fit(geo, e["n"], e["np"], 0) == (e["cpw"], e["nw"], e["lds"]) and e["tile"] == 512 // e["cpw"], e["name"]
            assert pc_geometry(geo, e["n"], e["np"], 0, e["channels"], pc.CUS, e["ts"])[4] == e["nseg"], e["name"]
        else:
            assert dec_fit(e["f32"], e["np"], e["D"], e["nout"]) == (e["cpw"], e["nw"], e["opl"], e["lds"]) and e["tile"] == e["opl"] * 64 // e["cpw"], e["name"]
            assert dec_geometry(e["f32"], e["D"], e["np"], e["nout"], e["channels"], pc.CUS, 0)[4] == e["nseg"] and e["al"] == dec.al_of(e["f32"], e["D"]), e["name"]
        d = cases.data(e)
        assert d["x"].shape == (e["channels"], cases.total(e)) == d["xq"].shape and d["pairs"].shape == d["x"].shape + (2,), e["name"]
        if e["stream"] == "parent":
            pd = (pc if e["kind"] == "pc" else dec)._data(cases.shape_of(e)[1:-1])
            assert d["x"] is pd["x"] and d["ti"] is pd["ti"], e["name"]
        for c in cases.burst_receivers(e):
            assert (d["x"][c, -3:] == cases.BURST_LEVEL).all() and np.abs(d["x"][c, :-3]).max() <= cases.QUIET and d["steps"][c] == 0 and d["modes"][c] == cases.AM, (e["name"], c)
        assert len(cases.burst_receivers(e)) >= (e["part"] in "DF"), e["name"]


def test_the_gain_launchers_are_the_plain_ones_with_the_gain_twins():
    """validation, geometry and LDS as the plain twins have them: each gain launcher's text is its plain twin's with the changes that make it the gain's"""
    seen = 0
    for real_src, gain_src, lds in (("msdr_chain_ncopc.hip", "msdr_chain_gncopc.hip", ("return f32pcn_lds_bytes(p.np, cpw, nw);", "return pcn_lds_bytes(p.np, cpw, nw);")),
                                    ("msdr_chain_decpc.hip", "msdr_chain_gdecpc.hip", ("return dec_launch(", "return dec_launch("))):
        real, gain = launchers(source(real_src)), launchers(source(gain_src))
        assert sorted(gain) == sorted(n + "_gain" for n in real) and len(gain) == 2, (sorted(real), sorted(gain))
        for (name, (args, body)), fn in zip(sorted(real.items()), lds):
            args, blocks = re.subn(r"\b(Pc\w*?)Params p\b", r"bool cx, \1GainParams p", args)
            body, agc = re.subn(r"p\.sin_tab && ", "p.sin_tab && p.agc && ", body)
            body, valid = re.subn(r"(iq_ok\(p, p\.n(?: / \(D > 0 \? D : 1\))?\))", r"\1 && (!cx || cx_ok(p.x, p.hist_in, p.cx_dir))", body)
            body, twins = re.subn(r"if \(p\.iq\) return p\.meter \? (chain_\w+?)_iq_meter_kernel(<[^>]*>) : \1_iq_kernel\2; return p\.meter \? \1_meter_kernel\2 : \1_kernel\2;",
                                  r"return cx ? \1_cx_gain_kernel\2 : \1_gain_kernel\2;", body)
            assert (blocks, agc, valid, twins) == (1, 1, 1, 1) and gain[name + "_gain"] == (args, body), (name, gain[name + "_gain"], (args, body))
            assert fn in body, name
            seen += 1
    assert seen == 4
    shared = source("msdr_pc_launch.h")
    assert "return dec_lds_bytes(f32, p.np, p.dec, cpw, nw, opl);" in shared and shared.count("dec_lds_bytes") == 1


def burst_rule(e, want):
    for c in cases.burst_receivers(e):
        print("%s ch %d longer %d true %d" % (e["name"], c, want["longer"][c], want["true"][c]))
        assert want["longer"][c] > 4 * want["true"][c] > 0, (e["name"], c, want["longer"][c], want["true"][c])


def q15_corners(orc, e, want):
    """part C, Q15: every named corner, from the model's own streams"""
    d, idx = cases.data(e), cases.out_index(e)
    xi, xq, si, sq = q15.streams(e)
    sat = lambda v: np.clip(v, -32768, 32767)          # noqa: E731
    prod = lambda a, b: sat((a.astype(np.int64) * b.astype(np.int64)) >> 15)          # noqa: E731
    seen = dict(wrap_gain=0, wrap_negative=0, zero=0, high=0, low=0, second=0)
    for c in range(e["channels"]):
        g, pairs = e["gains"][c], want["pairs"][c].astype(np.int32)
        if c % 4 < 2:          # the accumulator before it wraps
            wrapped = 0
            for k, (m, t) in enumerate(zip(M.mixed_q15(orc, xi[c], None if xq is None else xq[c], si[c], sq[c], e["dir"]), (d["ti"][c], d["tq"][c]))):
                true = np.convolve(m.astype(np.int64), t[::-1].astype(np.int64))[:m.size][idx]
                wrapped += int(np.abs(true).max() >= 1 << 31 and not np.array_equal(true, want["bank"].acc[c][k][idx].astype(np.int64)))
            assert wrapped, (e["name"], c)          # (with complex input one of the two mixed streams may cancel to zero)
            seen["wrap_gain" if g > 0 else "wrap_negative"] += 1
            if e["cx"] and c % 4 == 1:          # freq_conv's second saturation: a sum of two saturated products outside int16
                sign = -1 if e["dir"] else 1
                raw_i, raw_q = prod(xi[c], sq[c]) + sign * prod(xq[c], si[c]), prod(xq[c], sq[c]) - sign * prod(xi[c], si[c])
                seen["second"] += int((np.abs(raw_i) > 32768).any() or (np.abs(raw_q) > 32768).any())
        elif c % 4 == 2:
            assert g == 0.0 and M.multiplier(g) == 0 and not pairs.any() and not want["audio"][c].any(), (e["name"], c)
            seen["zero"] += 1
        else:
            seen["high"] += int((pairs == 32767).any())
            seen["low"] += int((pairs == -32768).any())
    print(e["name"], seen)
    assert all(v > 0 for k, v in seen.items() if k != "second") and (seen["second"] > 0) == e["cx"], (e["name"], seen)


@pytest.mark.parametrize("name", cases.names(0))
def test_q15_entry_in_the_model(name):
    e = cases.BY_NAME[name]
    orc = oracle()
    want = q15.model_q15(orc, e)
    live = [c for c in range(e["channels"]) if M.multiplier(e["gains"][c]) != 0 and not (e["stream"] == "corners" and c % 4 < 2)]          # (what a wrap leaves may be small)
    assert all(want["pairs"][c].any() for c in range(e["channels"]) if M.multiplier(e["gains"][c]) != 0), name
    assert all(np.abs(want["audio"][c].astype(np.int32)).max() > 100 and np.abs(want["pairs"][c].astype(np.int32)).max() > 100 for c in live), name
    assert (want["meters"] > 0).all() and len(want["words"]) == 4, name
    assert all(int(w[4]) == 3 * e["agc"][c] for c, w in enumerate(want["words"][-1]))
    if e["part"] == "B":          # the multiplier changes between the calls (a receiver inside the AGC's dead band keeps its own)
        moved = [c for c in live if len({int(w[c][0]) for w in want["words"]}) > 1]
        print("%s: the multiplier of %d of %d receivers changes" % (name, len(moved), e["channels"]))
        assert 2 * len(moved) >= e["channels"], (name, moved)
    if e["stream"] == "corners":
        q15_corners(orc, e, want)
    burst_rule(e, want)


@pytest.mark.parametrize("name", cases.names(1))
def test_fp32_entry_in_the_model(name):
    e = cases.BY_NAME[name]
    want = fp32.model_f32(oracle(), e)
    zero = tuple(c for c in range(e["channels"]) if e["gains"][c] == 0.0)
    print("%s: %d of %d receivers not judged by the float64 clause" % (name, len(e["unjudged"]), e["channels"]))
    assert e["unjudged"] == zero and 4 * len(zero) <= e["channels"], (name, zero)
    for c in range(e["channels"]):
        if c in zero:
            assert not want["audio32"][c].any() and not want["pairs"][c].any(), (name, c)
            continue
        e_orc, e_iq = rel(want["audio32"][c], want["audio64"][c]), float(np.sqrt((want["audio64"][c] ** 2).mean()))
        print("%s ch %d e_orc %.3e float64 rms %.3e" % (name, c, e_orc, e_iq))
        assert e_orc < 2e-6 and e_iq > 1e-4, (name, c, e_orc, e_iq)
    assert (want["meters"] > 0).all() and all(int(w[4]) == 3 * e["agc"][c] for c, w in enumerate(want["words"][-1])), name
    if e["part"] == "B":
        moved = [c for c in range(e["channels"]) if len({int(w[c][0]) for w in want["words"]}) > 1]
        print("%s: the multiplier of %d of %d receivers changes" % (name, len(moved), e["channels"]))
        assert 2 * len(moved) >= e["channels"], (name, moved)
    if e["part"] == "C":
        big = [c for c in range(e["channels"]) if e["gains"][c] == 1e6]
        loud = [c for c in range(e["channels"]) if e["gains"][c] == 40.0]
        assert big and loud and zero and min(e["gains"]) < 0 and all(M.clamped(e["gains"][c]) == np.float32(32767.0) for c in big), name
        for c in loud:          # the peak over in_scale passes 32767: absmax clamps
            s = cases.call_slices(e)[-1]
            assert float(np.abs(want["pairs"][c][s]).max()) / float(M.IN_SCALE) > 32767.0 and want["true"][c] == 32767, (name, c)
    burst_rule(e, want)
