"""The conditions on the table of the census of the complex-input chain kernels (tests/cx_census_cases.py), checked without a GPU:

  * the table is every q15pcn / f32pcn entry of tests/pc_census_cases.py and every entry of tests/decim_census_cases.py, each with its parent's
    fields unchanged, a unique name "cx-" + the parent's and a direction; the kernels of the table are the __global__ names of
    msdr_chain_cxpc.hiph, and the entries reach every instantiation the two cx launchers can select: 4 templates x 3 CPW per arithmetic for the
    sliding window, 4 x 12 (CPW, AL) pairs for Q15 and 4 x 9 for fp32 behind a decimator (AL = 0 is never selected for fp32: from the text of
    launch_chain_f32pcnd_cx) -- 108; each of the 16 templates is met with both directions; no entry exceeds the parents' cap of oracle work;
  * the geometry is not re-derived because the cx launchers ARE the real ones: the text of every launch_chain_*_cx is its real twin's with the
    parameter block's type, the kernels' names (the _cx twin of the same suffix under the same p.iq / p.meter) and cx_ok() in the validity
    changed -- the same LDS functions (pcn_lds_bytes, f32pcn_lds_bytes, dec_lds_bytes through dec_launch), the same read-width expressions;
  * every fp32 entry, row by row, with the oracle and float64 alone: e_orc < 2e-6 on the audio and on the pairs -- the clause of
    cx_cases.judge_f32 that keeps its other two honest -- and the float64 output has an rms above 1e-3; every figure is printed;
  * every Q15 row's expected audio, I and Q exceed 100 somewhere and every expected meter value is above 0; and at least one entry has a sum of
    two products outside int16 whose mixed sample sits at the rail (freq_conv's second saturation)."""
import os
import re

import numpy as np
import pytest

import cx_census_cases as cases
import decim_census_cases as dec
import pc_census_cases as pc
import test_gpu_cx_census as q15
import test_gpu_cx_census_f32 as fp32
from cx_cases import rel
from f32judge import oracle
from test_decim_geometry import CSRC

ENTRIES = cases.ENTRIES
PAIRS = {f32: {(cpw, dec.al_of(f32, D)) for cpw in (4, 2, 1) for D in range(2, dec.MAX_D[f32] + 1)} for f32 in (0, 1)}


def source(name):
    return open(os.path.join(CSRC, name)).read()


def launchers(text):
    """name -> (arguments, body) of every launch_chain_* function of a translation unit, comments and line breaks removed"""
    squeeze = lambda s: " ".join(re.sub(r"//[^\n]*", "", s).split())          # noqa: E731
    return {n: (squeeze(a), squeeze(b)) for n, a, b in re.findall(r"^hipError_t (launch_chain_\w+)\(([^)]*)\)\n\{\n(.*?)\n\}\n", text, re.S | re.M)}


def test_the_table_is_the_parents_entries():
    parents = [p for p in pc.ENTRIES if p["fam"] in cases.PC_FAMS] + list(dec.ENTRIES)
    assert len(ENTRIES) == len(parents) == len(set(cases.NAMES)) and len(dec.ENTRIES) == 244
    assert {p["fam"] for p in pc.ENTRIES if "pcn" in p["fam"]} == set(cases.PC_FAMS)
    for i, (e, p) in enumerate(zip(ENTRIES, parents)):
        assert e["name"] == "cx-" + p["name"] == "cx-" + e["parent"] and cases.parent_of(e) is p and e["dir"] == i % 2, e["name"]
        assert all(e[k] == v for k, v in p.items() if k != "name"), e["name"]
        assert set(e) - set(p) <= {"parent", "kind", "dir", "inmap", "warm", "ts"} and (e["kind"] == "pc" or (e["inmap"], e["warm"], e["ts"]) == (False, 0, 0)), e["name"]
        assert cases.work(e) <= cases.WORK_CAP == dec.WORK_CAP == pc.WORK_CAP, (e["name"], cases.work(e))
        d, pd = cases.data(e), (pc if e["kind"] == "pc" else dec).data(p)
        assert d["x"] is pd["x"] and d["ti"] is pd["ti"] and d["n"] == cases.total(e) == cases.out_index(e)[-1] + 1, e["name"]
        assert d["xq"].shape == d["x"].shape and d["pairs"].shape == d["x"].shape + (2,) and d["pairs"].dtype == np.int16, e["name"]
        assert np.array_equal(d["pairs"][..., 0], d["x"]) and np.array_equal(d["pairs"][..., 1], d["xq"]) and not d["pairs_q0"][..., 1].any(), e["name"]
        assert np.abs(d["xq"].astype(np.int32)).max() <= cases.AMP[e["f32"]] < 2 * np.abs(d["xq"].astype(np.int32)).max(), e["name"]
        assert not np.array_equal(d["xq"], d["x"]) and sum(cases.calls(e)) == len(cases.out_index(e)), e["name"]
    # the parts the issue of this census names: input maps, limits with a refusal, time segments of both kinds, full histories
    mine = lambda **kw: [e for e in ENTRIES if all(e.get(k) == v for k, v in kw.items())]          # noqa: E731
    assert len(mine(inmap=True)) == 2 and {e["f32"] for e in mine(inmap=True)} == {0, 1}
    assert {(e["f32"], e["ts"]) for e in mine(kind="pc", part="E")} == {(0, 0), (1, 0), (1, 3)} and all(e["n"] == pc.LONG for e in mine(kind="pc", part="E"))
    assert len(mine(kind="pc", part="F")) > 0 and all(e["warm"] == e["np"] + 1 for e in mine(kind="pc", part="F"))
    assert len(mine(part="D")) == 2 + 7 and all(e["refuse"] is not None for e in mine(part="D"))
    assert sum(e["at_cap"] for e in ENTRIES) >= 4 and any(e["at_cap"] for e in mine(kind="pc")) and any(e["at_cap"] for e in mine(kind="dec"))
    print("%d entries (%d sliding-window, %d decimating; %d Q15, %d fp32)" %
          (len(ENTRIES), len(mine(kind="pc")), len(mine(kind="dec")), len(cases.names(0)), len(cases.names(1))))


def test_every_instantiation_is_reached_in_both_directions():
    found = re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", source("msdr_chain_cxpc.hiph"))
    templates = {cases.template_of(e) for e in ENTRIES}
    assert len(found) == len(set(found)) == 16 and set(found) == templates, (found, sorted(templates))
    # what the launchers can select: pc_dispatch_cpw gives CPW 4 / 2 / 1; AL from the factor.  launch_chain_f32pcnd_cx never passes AL = 0 and
    # maps dec_dispatch_al's slot for it to the AL = 1 kernel again: 12 pairs for Q15, 9 for fp32
    body = launchers(source("msdr_chain_cxdecpc.hip"))
    assert "(D & 1) ? 0 : (D % 8 == 0) ? 4 : (D % 4 == 0) ? 2 : 1" in body["launch_chain_q15pcnd_cx"][1]
    assert "(D % 4 == 0) ? 4 : (D % 2 == 0) ? 2 : 1" in body["launch_chain_f32pcnd_cx"][1] and "(D & 1) ? 0" not in body["launch_chain_f32pcnd_cx"][1]
    assert "AL = decltype(a)::value == 0 ? 1 : decltype(a)::value" in body["launch_chain_f32pcnd_cx"][1]
    assert len(PAIRS[0]) == 12 and len(PAIRS[1]) == 9 and all(al != 0 for _, al in PAIRS[1])
    want = set()
    for f32 in (0, 1):
        for twin in cases.TWINS:
            want |= {("chain_%spcn_cx%s_kernel" % (cases.ARITH[f32], twin), cpw, None) for cpw in (4, 2, 1)}
            want |= {("chain_%spcnd_cx%s_kernel" % (cases.ARITH[f32], twin), cpw, al) for cpw, al in PAIRS[f32]}
    reached = {cases.instantiation(e) for e in ENTRIES}
    print("%d instantiations reached (Q15 %d, fp32 %d)" % (len(reached), sum("q15" in k[0] for k in reached), sum("f32" in k[0] for k in reached)))
    assert reached == want and len(want) == 108 and sum("q15" in k[0] for k in want) == 60, (sorted(want - reached), sorted(reached - want))
    for t in sorted(templates):
        assert {e["dir"] for e in ENTRIES if cases.template_of(e) == t} == {0, 1}, t


def test_the_cx_launchers_are_the_real_ones_with_the_cx_twins():
    """LDS, limits and read widths are the real kernels' own: each cx launcher's text is its real twin's, with the three changes that make it cx"""
    seen = 0
    for real_src, cx_src, lds in (("msdr_chain_ncopc.hip", "msdr_chain_cxncopc.hip", ("return f32pcn_lds_bytes(p.np, cpw, nw);", "return pcn_lds_bytes(p.np, cpw, nw);")),          # (sorted by name: f32 first)
                                  ("msdr_chain_decpc.hip", "msdr_chain_cxdecpc.hip", ("return dec_launch(", "return dec_launch("))):
        real, cx = launchers(source(real_src)), launchers(source(cx_src))
        assert sorted(cx) == sorted(n + "_cx" for n in real) and len(cx) == 2, (sorted(real), sorted(cx))
        for (name, (args, body)), fn in zip(sorted(real.items()), lds):
            args = re.sub(r"\b(Pc\w*?)Params\b", r"\1CxParams", args)
            body, twins = re.subn(r"\b(chain_(?:q15|f32)pcnd?)((?:_iq)?(?:_meter)?)_kernel\b", r"\1_cx\2_kernel", body)
            body, valid = re.subn(r"(iq_ok\(p, p\.n(?: / \(D > 0 \? D : 1\))?\))", r"\1 && cx_ok(p.x, p.hist_in, p.cx_dir)", body)
            assert (twins, valid) == (4, 1) and cx[name + "_cx"] == (args, body), (name, cx[name + "_cx"], (args, body))
            assert fn in body and re.search(r"if \(p\.iq\) return p\.meter \? chain_\w+_cx_iq_meter_kernel<[^>]*> : chain_\w+_cx_iq_kernel<[^>]*>; "
                                            r"return p\.meter \? chain_\w+_cx_meter_kernel<[^>]*> : chain_\w+_cx_kernel<[^>]*>;", body), name
            seen += 1
    assert seen == 4
    shared = source("msdr_pc_launch.h")
    assert "return dec_lds_bytes(f32, p.np, p.dec, cpw, nw, opl);" in shared and shared.count("dec_lds_bytes") == 1


@pytest.mark.parametrize("name", cases.names(1))
def test_fp32_oracle_is_inside_the_judge(name):
    e = cases.BY_NAME[name]
    idx = cases.out_index(e)
    for c, (w32, w64) in enumerate(fp32.refs_f32(oracle(), e)):
        e_orc, e_iq = rel(w32[0][idx], w64[0][idx]), rel(*fp32.iq_rows((w32, w64), idx))
        rms = float(np.sqrt((w64[0][idx] ** 2).mean()))
        print("%s row %d e_orc %.3e pairs %.3e float64 rms %.3e" % (name, c, e_orc, e_iq, rms))
        assert e_orc < 2e-6 and e_iq < 2e-6, (name, c, e_orc, e_iq)
        assert rms > 1e-3, (name, c, rms)
    if "meter" in e["twin"]:
        assert all(float((env[k].astype(np.float64) ** 2).sum()) > 0 for env in fp32.refs_env(oracle(), e) for k in q15.meter_index(e)), name


def rails(e, refs):
    """samples whose sum of two (already saturated) products leaves int16, over the entry's channels; the mixed sample then sits at the rail"""
    d = cases.data(e)
    n128 = refs[0][3].size
    si, sq = q15.oscillator(e, n128)
    xi, xq = (q15.padded(cases.heard(e, d[k]), n128) for k in ("x", "xq"))
    sat = lambda v: np.clip(v, -32768, 32767)          # noqa: E731
    p = lambda a, b: sat((a.astype(np.int64) * b.astype(np.int64)) >> 15)          # noqa: E731
    raw_i = p(xi, sq) + (-1 if e["dir"] else 1) * p(xq, si)
    over = (raw_i > 32767) | (raw_i < -32768)
    mixed_i = np.stack([w[3] for w in refs])
    assert np.array_equal(mixed_i, sat(raw_i).astype(np.int16)) and np.isin(mixed_i[over], (32767, -32768)).all(), e["name"]
    return int(over[:, :d["n"]].sum())


@pytest.mark.parametrize("name", cases.names(0))
def test_q15_rows_are_not_degenerate(name):
    e = cases.BY_NAME[name]
    idx = cases.out_index(e)
    refs = q15.refs_q15(oracle(), e)
    for c, w in enumerate(refs):
        assert all(np.abs(r[idx].astype(np.int32)).max() > 100 for r in w[:3]), (name, c)
        assert all(int((w[1][k].astype(np.int64) ** 2 + w[2][k].astype(np.int64) ** 2).sum()) > 0 for k in q15.meter_index(e)), (name, c)
    print("%s: %d sums outside int16" % (name, rails(e, refs)))


def test_the_second_saturation_is_met():
    """from the oracle alone, on the cheapest Q15 entries of both halves and both directions"""
    met = {}
    for kind in ("pc", "dec"):
        for direction in (0, 1):
            e = min((e for e in ENTRIES if not e["f32"] and e["kind"] == kind and e["dir"] == direction), key=lambda e: (cases.work(e), e["name"]))
            met[e["name"]] = rails(e, q15.refs_q15(oracle(), e))
    print(met)
    assert sum(v > 0 for v in met.values()) >= 1, met
