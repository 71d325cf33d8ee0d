"""The conditions on the table of the census of the sliding-window per-receiver kernels (tests/pc_census_cases.py), checked without a GPU:

  * part A names exactly the launch geometries the rule can reach -- brute force over every family, every filter length its setter accepts and
    the call lengths -- so a change of pc_fit_lds without a table entry turns this red; and every entry's geometry is what pc_geometry ITSELF
    computes from the kernels' own sizing functions (a probe compiled against msdr_pc_geometry.h and the four kernel headers, host code only), so
    the figures the GPU cases assert against chain.info() are the launcher's, not only the restated rule's;
  * the kernels of the table are the __global__ names of the four kernel headers, and parts A + B hold every (instantiation, CPW) pair the four
    launchers can select: 60;
  * no entry asks more than 2e8 multiply-adds of the oracle, no call length is a multiple of a tile, every entry has a partial channel group;
  * every part-A shape whose filter is longer than its three calls is in part F behind a call that fills the history;
  * every fp32 entry, row by row, with the oracle and float64 alone: 2 e_orc + fp32_noise + 1e-6 < 5e-6 (the cap of
    tests/test_f32_flavour_cases.py and of the decimation census, half of the 1e-5 clause), and the float64 output is not degenerate; every Q15
    row, I and Q exceeds 100 somewhere and every expected meter value is above 0;
  * part D's figures are the setters' own functions (f32pc_max_taps, pcn_max_taps / f32pcn_max_taps, pco_max_taps / f32pco_max_taps and the
    interface's 4096), read through the probe, and the entries the LDS formula puts at exactly 65 536 bytes say so."""
import os
import re
import subprocess

import numpy as np
import pytest
from scipy.signal import lfilter

import pc_census_cases as cases
import test_gpu_pc_census as q15
import test_gpu_pc_census_f32 as fp32
from f32judge import fp32_noise, oracle
from gpuhelp import rel_rms
from test_gpu_meter_per_channel import sums
from test_pc_geometry import CAP, CSRC, geometry, lds_bytes

ENTRIES = cases.ENTRIES
HEADERS = ("msdr_chain_q15pc.hiph", "msdr_chain_f32pc.hiph", "msdr_chain_oscpc.hiph", "msdr_chain_ncopc.hiph")
LAUNCHERS = ("msdr_chain_q15pc.hip", "msdr_chain_f32pc.hip", "msdr_chain_oscpc.hip", "msdr_chain_ncopc.hip")
PROBE = r"""
#include <cstdio>
#include <cstdlib>
#include "msdr_chain_ncopc.hiph"
int main(int argc, char **argv)
{
    using namespace msdr;
    const int l1 = atoi(argv[1]), l2 = atoi(argv[2]);
    printf("%d %d %d %d %d %d %d %d %d %d\n", f32pc_max_taps(false), f32pc_max_taps(true), pcn_max_taps(), f32pcn_max_taps(), pco_max_taps(128),
           f32pco_max_taps(128), pco_max_taps(l1), f32pco_max_taps(l2), pco_max_taps(l1 + 1), f32pco_max_taps(l2 + 1));
    int f, np, o, ch, ts; long long n;
    while (scanf("%d %d %d %lld %d %d", &f, &np, &o, &n, &ch, &ts) == 6) {
        PcGeometry g;
        auto bytes = [&](int cpw, int nw) -> size_t {
            switch (f) {
            case 0: return pc_lds_bytes(np, cpw, false, nw);
            case 1: return pc_lds_bytes(np, cpw, true, nw);
            case 2: return f32pc_lds_bytes(np, cpw, false, false, nw);
            case 3: return f32pc_lds_bytes(np, cpw, false, true, nw);
            case 4: return f32pc_lds_bytes(np, cpw, true, false, nw);
            case 5: return pco_lds_bytes(np, o, cpw, nw);
            case 6: return f32pco_lds_bytes(np, o, cpw, nw);
            case 7: return pcn_lds_bytes(np, cpw, nw);
            default: return f32pcn_lds_bytes(np, cpw, nw);
            }
        };
        if (!pc_geometry(n, ch, 256, ts, f == 1 || f == 0 || f == 5 || f == 7 ? kPcR : kPfR, kPcLdsCap, bytes, &g)) { printf("refused\n"); continue; }
        printf("%d %d %zu %d %u %u %d\n", g.launch.cpw, g.nw, g.launch.lds_bytes, g.launch.tile, g.launch.block, g.launch.grid, g.launch.nseg);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """(the setters' limits, one line of geometry per entry) from the headers themselves"""
    d = tmp_path_factory.mktemp("pc_census")
    src, exe = str(d / "probe.hip"), str(d / "probe")
    with open(src, "w") as f:
        f.write(PROBE)
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-fwrapv", "-Wno-unused-value", "-I" + CSRC, "-o", exe, src])
    asked = "".join("%d %d %d %d %d %d\n" % (cases.FAM_NAMES.index(e["fam"]), e["np"], e["osc"], e["n"], e["channels"], e["ts"]) for e in ENTRIES)
    lines = subprocess.run([exe, str(cases.longest_row("q15pco")), str(cases.longest_row("f32pco"))], input=asked, check=True, capture_output=True,
                           text=True).stdout.splitlines()
    assert len(lines) == 1 + len(ENTRIES)
    return [int(v) for v in lines[0].split()], lines[1:]


def test_part_a_is_every_reachable_geometry():
    seen = {}
    for f in cases.FAMS:
        fam, q = f["name"], cases.QUANT[f["f32"]]
        osc = cases.ROW_LEN if f["mixers"] == ("rows",) else 0
        top = cases.limit_of(fam, osc)
        assert q <= top <= 4096, fam
        for np_ in range(q, top + 1, q):
            for n in (29, 131, 259, 1, 2, 128, 129, 256, 257, 1 << 20):
                k = cases.key_of(fam, np_, n, osc)
                assert k is not None, (fam, np_, n)                      # (the setter's limit IS the rule's: nothing it accepts is refused)
                if n in cases.LENGTHS.values():
                    seen[k] = min(seen.get(k, 1 << 62), n * np_)
                else:
                    assert k in seen, k                                  # the three lengths stand for their classes
    part_a = [e for e in ENTRIES if e["part"] == "A" and e["osc"] != cases.ODD_LEN]
    rows = [(cases.key(e), e["mixer"]) for e in part_a]
    assert len(set(rows)) == len(rows) and {k for k, _ in rows} == set(seen), (sorted(set(seen) - {k for k, _ in rows}), sorted({k for k, _ in rows} - set(seen)))
    assert all({m for k, m in rows if k == key} == set(cases.FAM[key[0]]["mixers"]) for key in seen)          # every key under every mixer of its family
    per_fam = [sum(k[0] == fam for k in seen) for fam in cases.FAM_NAMES]
    lowered = sum(k[2] < k[1] for k in seen)
    print("reachable geometries: %d (%s); the fit lowers CPW in %d; part A has %d entries" %
          (len(seen), ", ".join("%s %d" % p for p in zip(cases.FAM_NAMES, per_fam)), lowered, sum(e["part"] == "A" for e in ENTRIES)))
    assert (len(seen), per_fam, lowered) == (105, [12, 9, 12, 12, 12, 12, 12, 12, 12], 25)
    for e in part_a:                                                     # the cheapest shape of its key; np == nt
        assert e["n"] * e["np"] == seen[cases.key(e)] and e["nt"] == e["np"] and e["twin"] == "", e["name"]
    assert {(k[1], k[2]) for k in seen if k[2] < k[1]} == {(4, 2), (4, 1), (2, 1)}
    assert all(e["tile"] > e["n"] for e in part_a if e["lowered"])       # the tile is then larger than the whole call
    # the tables whose length is no power of two: one per CPW on both families that read a table from global memory
    odd = [e for e in ENTRIES if e["osc"] == cases.ODD_LEN]
    assert sorted((e["fam"], e["cpw"]) for e in odd) == sorted((f, c) for f in ("q15pc", "f32pc") for c in (1, 2, 4)) and all(e["mixer"] == "tab" for e in odd)


def test_every_entry_has_the_geometry_the_header_computes(probe):
    for e, ln in zip(ENTRIES, probe[1]):
        cpw, nw, lds, tile, block, grid, nseg = (int(v) for v in ln.split())
        assert (cpw, nw, lds, tile, block, nseg) == (e["cpw"], e["nw"], e["lds"], e["tile"], 64 * e["nw"], e["nseg"]), (e["name"], ln)
        g = geometry(cases.FAM[e["fam"]]["geo"], e["n"], e["np"], cases.lds_osc(e["fam"], e["osc"]), e["channels"], 256, e["ts"])
        assert (grid, block, lds, cpw, nseg, tile, nw) == g[:6] + g[7:], (e["name"], ln, g)
        if e["part"] != "E":
            assert (grid, nseg) == (2, 1), (e["name"], ln)               # one full workgroup, one with a single valid channel group; one segment
        else:                                                            # waves + 1 channel groups x 2 or 3 segments: with two waves, units of different groups and segments in one workgroup
            assert nseg == (3 if e["ts"] == 3 else 2) and grid == -(-(nw + 1) * nseg // nw), (e["name"], ln)


def test_names_kernels_and_instantiations():
    assert len(set(cases.NAMES)) == len(ENTRIES)
    found = []
    for h in HEADERS:
        found += re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", open(os.path.join(CSRC, h)).read())
    table = {cases.kernel_name(e["fam"], e["twin"]) for e in ENTRIES}
    assert len(found) == len(set(found)) == 16 and set(found) == table, (found, sorted(table))
    # every instantiation the four launchers can select: the kernel and the template arguments behind CPW, from the launchers' source text;
    # pc_dispatch_cpw gives each of them CPW 4 / 2 / 1
    selected = set()
    for src in LAUNCHERS:
        text = open(os.path.join(CSRC, src)).read()
        assert text.count("pc_launch(") == text.count("hipError_t launch_chain_")
        selected |= {(k, a.replace("decltype(cpw)::value", "CPW")) for k, a in re.findall(r"\b(chain_\w+_kernel)<([^<>]*)>", text)}
    templates = {cases.template_of(f["name"], twin) for f in cases.FAMS for twin in f["twins"]}
    assert selected == {(k, "CPW" + a) for k, a in templates} and len(selected) == 20, (sorted(selected), sorted(templates))
    geo = open(os.path.join(CSRC, "msdr_pc_geometry.h")).read()
    assert all(s in geo for s in ("case 4: f(std::integral_constant<int, 4>())", "case 2: f(std::integral_constant<int, 2>())", "default: f(std::integral_constant<int, 1>())"))
    want = {(f["name"], twin, cpw) for f in cases.FAMS for twin in f["twins"] for cpw in (4, 2, 1)}
    ab = {(e["fam"], e["twin"], e["cpw"]) for e in ENTRIES if e["part"] in "AB"}
    counts = [sum(e["part"] == p for e in ENTRIES) for p in "ABCDEF"]
    print("part A %d, part B %d, part C %d, part D %d, part E %d, part F %d entries (%d Q15, %d fp32); %d distinct instantiations of pc_frame / pf_frame" %
          tuple(counts + [len(cases.names(0)), len(cases.names(1)), len(ab)]))
    assert ab == want and len(want) == 60
    assert counts == [123, 62, 85, 12, 50, 87] and len(ENTRIES) == 419
    # part B: every twin at every CPW, at a shape with fewer than four waves and at one whose CPW the fit lowered; an input map per chain family
    for f in cases.FAMS:
        for twin in f["twins"][1:]:
            mine = [e for e in ENTRIES if e["part"] == "B" and e["fam"] == f["name"] and e["twin"] == twin]
            assert len(mine) == 5 and {e["cpw"] for e in mine} == {4, 2, 1} and any(e["nw"] < 4 for e in mine) and any(e["lowered"] for e in mine), (f["name"], twin)
        maps = [e for e in ENTRIES if e["inmap"] and e["fam"] == f["name"]]
        assert len(maps) == (1 if f["chain"] else 0) and all(e["nw"] < 4 and e["twin"] == "" and e["part"] == "B" for e in maps), f["name"]


def test_the_recipe_and_the_cost_of_every_entry():
    assert all(n % t for n in list(cases.LENGTHS.values()) + [cases.LONG] for t in (128, 256, 512))          # every call ends in a partial tile
    assert all(n % 2 for n in cases.LENGTHS.values())                    # odd: the rows of odd channels start at odd element offsets
    for e in ENTRIES:
        f = cases.FAM[e["fam"]]
        assert cases.work(e) <= cases.WORK_CAP, (e["name"], cases.work(e))
        assert e["channels"] == min(17, e["cpw"] * e["nw"] + 1) and e["channels"] % e["cpw"] == 1 % e["cpw"], e["name"]
        assert e["warm"] == (e["np"] + 1 if e["part"] == "F" else 0) and e["warm"] % 2 == (e["part"] == "F")          # (odd: no multiple of a tile)
        assert e["n"] == (cases.LONG if e["part"] == "E" else cases.LENGTHS[e["cls"]]) and e["np"] == cases.padded(e["f32"], e["nt"]), e["name"]
        assert e["lds"] == lds_bytes(f["geo"], e["np"], cases.lds_osc(e["fam"], e["osc"]), e["cpw"], e["nw"]) <= CAP and e["tile"] == 512 // e["cpw"], e["name"]
        d = cases.data(e)
        assert d["x"].shape == (e["channels"], e["warm"] + 2 * e["n"] + 2) == (e["channels"], sum(cases.calls(e))) and d["ti"].shape == (e["channels"], e["nt"]), e["name"]
        assert len(set(d["steps"].tolist())) == e["channels"] and (np.all(d["ti"] != 0) or e["nt"] >= 16), e["name"]
        if e["mixer"] == "rows":
            assert d["oi"].shape == (e["channels"], e["osc"]) and len({r.tobytes() for r in d["oi"]}) == e["channels"], e["name"]
    print("the dearest entry: %s, %d multiply-adds" % max((cases.work(e), e["name"]) for e in ENTRIES)[::-1])
    # part C: 131 samples, np exact and padded by every remainder (Q15: even counts), the one-tap filter and all residues of the step count mod 3 (fp32)
    for f in cases.FAMS:
        for mixer in f["mixers"]:
            mine = [e for e in ENTRIES if e["part"] == "C" and e["fam"] == f["name"] and e["mixer"] == mixer]
            assert all(e["n"] == 131 for e in mine) and {e["np"] - e["nt"] for e in mine} == ({0, 1, 2, 3} if f["f32"] else {0, 2, 6}), (f["name"], mixer)
            assert {e["np"] // cases.QUANT[f["f32"]] for e in mine} >= {1, 2}
            if f["f32"]:
                assert {(e["np"] // 4) % 3 for e in mine} == {0, 1, 2} and any(e["nt"] == 1 for e in mine), (f["name"], mixer)
    # part F: exactly the part-A shapes (both mixers of the Q15 chain) whose filter is longer than the three calls -- among them every key with
    # fewer than four waves -- under the same geometry, behind a call as long as the filter
    part_a = {e["name"][1:]: e for e in ENTRIES if e["part"] == "A" and e["osc"] != cases.ODD_LEN}
    part_f = {e["name"][1:]: e for e in ENTRIES if e["part"] == "F"}
    assert set(part_f) == {k for k, e in part_a.items() if e["np"] > 2 * e["n"] + 2} >= {k for k, e in part_a.items() if e["nw"] < 4}
    assert all(cases.key(e) == cases.key(part_a[k]) and (e["np"], e["mixer"], e["twin"]) == (part_a[k]["np"], part_a[k]["mixer"], "") for k, e in part_f.items())
    assert all(e["warm"] >= e["np"] for e in part_f.values())
    # part E: one channel per wave, 2 and 1 waves, 9 tiles in 2 segments (the rule) or 3 (time_segments; fp32 only); plain, metered and I/Q kernels
    for f in cases.FAMS:
        mine = [e for e in ENTRIES if e["part"] == "E" and e["fam"] == f["name"]]
        want = {(nw, ts, twin) for nw in (2, 1) for ts in ((0, 3) if f["f32"] else (0,)) for twin in f["twins"][:3]} if f["chain"] else set()
        assert {(e["nw"], e["ts"], e["twin"]) for e in mine} == want and len(mine) == len(want), f["name"]
        assert all(e["cpw"] == 1 and -(-e["n"] // 512) == 9 and e["nseg"] == (3 if e["ts"] else 2) for e in mine), f["name"]


def test_part_d_is_the_setters_limit(probe):
    f32pc, f32fir, pcn, f32pcn, pco, f32pco, pco_long, f32pco_long, pco_past, f32pco_past = probe[0]
    launcher = open(os.path.join(CSRC, "msdr_chain_ncopc.hip")).read()
    assert "int chain_pcn_max_taps(bool f32) { return f32 ? f32pcn_max_taps() : pcn_max_taps(); }" in launcher
    l1, l2 = cases.longest_row("q15pco"), cases.longest_row("f32pco")
    assert pco_long >= 8 > pco_past and f32pco_long >= 4 > f32pco_past          # the longest rows that still leave a filter
    limits = {("q15pc", 0): 4096, ("q15pc", 128): 4096, ("q15fir", 0): 4096, ("f32pc", 128): f32pc, ("f32fs4", 0): f32pc, ("f32fir", 0): min(f32fir, 4096),
              ("q15pco", 128): min(pco, 4096), ("q15pco", l1): pco_long, ("f32pco", 128): f32pco, ("f32pco", l2): f32pco_long, ("q15pcn", 0): min(pcn, 4096),
              ("f32pcn", 0): f32pcn}
    part_d = [e for e in ENTRIES if e["part"] == "D"]
    assert {(e["fam"], e["osc"]) for e in part_d} == set(limits) and len(part_d) == len(limits)
    assert f32fir > 4096 and pco > 4096 and pcn > 4096                     # (there the interface's 4096 is the limit)
    for e in part_d:
        q = cases.QUANT[e["f32"]]
        assert e["nt"] == e["np"] == limits[(e["fam"], e["osc"])] and e["n"] == 131, e["name"]
        assert e["refuse"] == (None if cases.FAM[e["fam"]]["limit"] is None else e["nt"] + q), e["name"]
        assert (e["cpw"], e["nw"]) == (1, 1) or not e["chain"], e["name"]
        assert e["at_cap"] == (e["lds"] == 65536) == e["name"].endswith("-lds65536"), e["name"]
        if e["refuse"] is not None and e["refuse"] <= 4096:              # one step up the rule refuses what the setter is asked for
            geo = cases.FAM[e["fam"]]["limit"]
            assert lds_bytes(geo, e["refuse"], cases.lds_osc(e["fam"], e["osc"]), 1, 1) > CAP, e["name"]
    assert sorted(e["name"] for e in part_d if e["at_cap"]) == sorted(["D-f32pc-nt3840-lds65536", "D-q15pco-osc15336-nt8-lds65536", "D-f32pco-osc128-nt3776-lds65536",
                                                                      "D-f32pco-osc7552-nt64-lds65536", "D-f32pcn-nt3584-lds65536"])


@pytest.mark.parametrize("name", cases.names(1))
def test_fp32_bound_is_tight_and_the_output_is_not_degenerate(name):
    e = cases.BY_NAME[name]
    if not e["chain"]:          # the stage's judge is 1e-6 against the oracle: the oracle itself must be well inside that of float64
        d = cases.data(e)
        for c, want in enumerate(fp32.refs_fir(oracle(), e)):
            truth = lfilter(d["ti"][c].astype(np.float64)[::-1], [1.0], d["x"][c].astype(np.float64))
            e_orc, rms = rel_rms(want, truth), float(np.sqrt((truth ** 2).mean()))
            print("%s row %d e_orc %.3e float64 rms %.3e" % (name, c, e_orc, rms))
            assert e_orc < 5e-7 and rms > 1e-3, (name, c, e_orc, rms)
        return
    refs = fp32.refs_f32(oracle(), e)
    for c in range(e["channels"]):
        want, truth, _ = refs[c]
        e_orc = rel_rms(want, truth)
        bound = 2 * e_orc + fp32_noise(None) + 1e-6
        rms = float(np.sqrt((truth ** 2).mean()))
        print("%s row %d e_orc %.3e bound %.3e float64 rms %.3e" % (name, c, e_orc, bound, rms))
        assert bound < 5e-6, (name, c, bound)
        assert rms > 1e-3, (name, c, rms)                                # (the input's rms is 0.35 of full scale)


@pytest.mark.parametrize("name", cases.names(0))
def test_q15_rows_are_not_degenerate(name):
    e = cases.BY_NAME[name]
    m = cases.total(e)
    for c, rows in enumerate(q15.refs_q15(oracle(), e)):
        assert all(np.abs(r[:m].astype(np.int32)).max() > 100 for r in rows), (name, c)
        if e["chain"]:
            lo = 0
            for n in cases.calls(e):
                assert sums(rows[1][lo:lo + n], rows[2][lo:lo + n], n, n)[0] > 0, (name, c, lo)
                lo += n
