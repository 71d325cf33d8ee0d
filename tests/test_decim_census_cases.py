"""The conditions on the table of the decimation census (tests/decim_census_cases.py), checked without a GPU:

  * part A names exactly the launch geometries the rule can reach -- brute force over every factor, every filter length and the call lengths --
    so a change of dec_geometry without a table entry turns this red; and every entry's geometry is what the HEADER itself computes (a g++
    probe over msdr_decpc_geometry.h), so the figures the GPU cases assert against chain.info() are the launcher's, not only the restated rule's;
  * the kernels of the table are the __global__ names of msdr_chain_decpc.hiph, and part B holds every (CPW, AL) pair each twin's launcher
    can select, and one entry whose CPW the fit lowered;
  * no entry asks more than 2e8 multiply-adds of the oracle, no call length is a multiple of a tile, every entry has a partial channel group;
  * every fp32 entry, row by row, with the oracle and float64 alone: 2 e_orc + fp32_noise + 1e-6 < 5e-6 (the cap of
    tests/test_f32_flavour_cases.py, half of the 1e-5 clause), and the float64 output is not degenerate; every Q15 row exceeds 100 somewhere;
  * part D's figures are max_taps(f, D) capped at 4096, and the entries the LDS formula puts at exactly 65 536 bytes say so."""
import os
import re
import subprocess

import numpy as np
import pytest

import decim_census_cases as cases
import test_gpu_decim_census as q15
import test_gpu_decim_census_f32 as fp32
from f32judge import fp32_noise, oracle
from gpuhelp import rel_rms
from test_decim_geometry import CAP, CSRC, fit, lds_bytes, max_taps

ENTRIES = cases.ENTRIES
PROBE = r"""
#include <cstdio>
#include "msdr_decpc_geometry.h"
int main()
{
    using namespace msdr;
    int f, D, np, ch; long long nout;
    while (scanf("%d %d %d %lld %d", &f, &D, &np, &nout, &ch) == 5) {
        DecGeometry g;
        auto bytes = [&](int cpw, int nw, int opl) { return dec_lds_bytes(f == 1, np, D, cpw, nw, opl); };
        if (!dec_geometry(nout, ch, 256, 0, kPcLdsCap, bytes, &g)) { printf("refused\n"); continue; }
        printf("%d %d %d %zu %d %u %u %d\n", g.launch.cpw, g.nw, g.opl, g.launch.lds_bytes, g.launch.tile, g.launch.block, g.launch.grid, g.launch.nseg);
    }
    return 0;
}
"""


def test_part_a_is_every_reachable_geometry():
    seen = {}
    for f32 in (0, 1):
        for D in range(2, cases.MAX_D[f32] + 1):
            top = min(max_taps(f32, D), 4096)
            assert top >= cases.QUANT[f32], (f32, D)                     # every factor of the interface's range holds the shortest filter
            for np_ in range(cases.QUANT[f32], top + 1, cases.QUANT[f32]):
                for nout in (30, 130, 258, 1, 2, 128, 129, 256, 257, 1 << 20):
                    g = fit(f32, np_, D, nout)
                    assert g is not None, (f32, D, np_, nout)            # (the setter's limit IS the rule's: nothing it accepts is refused)
                    k = (f32, 4 if nout <= 128 else 2 if nout <= 256 else 1, g[0], g[1], g[2], cases.al_of(f32, D))
                    if nout in cases.LENGTHS.values():
                        seen[k] = min(seen.get(k, 1 << 62), nout * D * np_)
                    else:
                        assert k in seen, k                 # the three lengths stand for their classes
    part_a = [e for e in ENTRIES if e["part"] == "A"]
    keys = [cases.key(e) for e in part_a]
    assert len(set(keys)) == len(keys) and set(keys) == set(seen), (sorted(set(seen) - set(keys)), sorted(set(keys) - set(seen)))
    lowered = [e for e in part_a if e["lowered"]]
    print("reachable geometries: %d (Q15 %d, fp32 %d); the fit lowers CPW in %d" % (len(seen), sum(not k[0] for k in seen), sum(k[0] for k in seen), len(lowered)))
    assert (len(seen), sum(not k[0] for k in seen), sum(k[0] for k in seen), len(lowered)) == (120, 69, 51, 21)
    for e in part_a:                                                     # the cheapest shape of its key, below 4e6; np == nt
        assert e["nout"] * e["D"] * e["np"] == seen[cases.key(e)] < 4 * 10 ** 6 and e["nt"] == e["np"] and e["twin"] == "", e["name"]
    assert {(e["cls"], e["cpw"]) for e in lowered} == {(4, 2), (4, 1), (2, 1)}
    assert all(e["tile"] > e["nout"] for e in lowered if e["cls"] == 4)  # from class 4 the tile is then larger than the whole call
    dearest = max(part_a, key=lambda e: e["nout"] * e["D"] * e["np"])
    assert (dearest["f32"], dearest["D"], dearest["np"], dearest["nout"]) == (0, 56, 264, 258), dearest


def test_every_entry_has_the_geometry_the_header_computes(tmp_path):
    src, exe = str(tmp_path / "probe.cpp"), str(tmp_path / "probe")
    with open(src, "w") as f:
        f.write(PROBE)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, "-o", exe, src])
    asked = "".join("%d %d %d %d %d\n" % (e["f32"], e["D"], e["np"], e["nout"], e["channels"]) for e in ENTRIES)
    lines = subprocess.run([exe], input=asked, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(ENTRIES)
    for e, ln in zip(ENTRIES, lines):
        cpw, nw, opl, lds, tile, block, grid, nseg = (int(v) for v in ln.split())
        assert (cpw, nw, opl, lds, tile, block) == (e["cpw"], e["nw"], e["opl"], e["lds"], e["tile"], 64 * e["nw"]), (e["name"], ln)
        assert (grid, nseg) == (2, 1), (e["name"], ln)                   # one full workgroup, one with a single valid channel group; one segment


def test_names_kernels_and_the_pairs_of_part_b():
    assert len(set(cases.NAMES)) == len(ENTRIES) == 244
    src = open(os.path.join(CSRC, "msdr_chain_decpc.hiph")).read()
    found = re.findall(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(", src)
    table = {cases.kernel_name(e["f32"], e["twin"]) for e in ENTRIES}
    assert len(found) == 8 and set(found) == table, (found, sorted(table))
    # the (CPW, AL) pairs a launcher can select: AL from the factor, CPW 4 / 2 / 1.  launch_chain_f32pcnd never passes AL = 0 (Q15's name for
    # the odd factors), and dec_dispatch_al's slot for it holds the AL = 1 kernel again: 12 pairs for Q15, 9 for fp32
    launcher = open(os.path.join(CSRC, "msdr_chain_decpc.hip")).read()
    assert "(D & 1) ? 0 : (D % 8 == 0) ? 4 : (D % 4 == 0) ? 2 : 1" in launcher and "(D % 4 == 0) ? 4 : (D % 2 == 0) ? 2 : 1" in launcher
    assert "AL = decltype(a)::value == 0 ? 1 : decltype(a)::value" in launcher
    pairs = {f32: {(cpw, cases.al_of(f32, D)) for cpw in (4, 2, 1) for D in range(2, cases.MAX_D[f32] + 1)} for f32 in (0, 1)}
    assert len(pairs[0]) == 12 and len(pairs[1]) == 9
    counts = []
    for f32 in (0, 1):
        assert {(e["cpw"], e["al"]) for e in ENTRIES if e["part"] == "A" and e["f32"] == f32} == pairs[f32]
        for twin in cases.TWINS[1:]:
            mine = [e for e in ENTRIES if e["part"] == "B" and e["f32"] == f32 and e["twin"] == twin]
            assert {(e["cpw"], e["al"]) for e in mine} == pairs[f32], (f32, twin)
            assert sum(e["lowered"] for e in mine) >= 1, (f32, twin)
            counts.append(len(mine))
    assert counts == [13, 13, 13, 10, 10, 10]
    instantiations = {(e["f32"], e["twin"], e["cpw"], e["al"]) for e in ENTRIES}
    print("part A %d, part B %d, part C %d, part D %d entries; %d distinct instantiations (Q15 4 x 12, fp32 4 x 9)" %
          tuple([sum(e["part"] == p for e in ENTRIES) for p in "ABCD"] + [len(instantiations)]))
    assert len(instantiations) == 4 * 12 + 4 * 9
    assert [sum(e["part"] == p for e in ENTRIES) for p in "ABCD"] == [120, 69, 48, 7]


def test_the_recipe_and_the_cost_of_every_entry():
    tiles = {opl * 64 // cpw for opl in (2, 4, 8) for cpw in (1, 2, 4)}
    assert all(n % t for n in cases.LENGTHS.values() for t in tiles)     # every call ends in a partial tile
    for e in ENTRIES:
        assert cases.work(e) <= cases.WORK_CAP, (e["name"], cases.work(e))
        assert e["channels"] == min(17, e["cpw"] * e["nw"] + 1) and e["channels"] % e["cpw"] == 1 % e["cpw"], e["name"]
        assert e["nout"] == cases.LENGTHS[e["cls"]] and e["np"] == cases.padded(e["f32"], e["nt"]) and e["lds"] <= CAP, e["name"]
        assert e["lds"] == lds_bytes(e["f32"], e["np"], e["D"], e["cpw"], e["nw"], e["opl"]), e["name"]
        d = cases.data(e)
        assert d["x"].shape == (e["channels"], (2 * e["nout"] + 2) * e["D"]) and len(set(d["steps"].tolist())) == e["channels"], e["name"]
        assert cases.out_index(e).size == 2 * e["nout"] + 2 and cases.out_index(e)[-1] == d["n"] - 1, e["name"]
        assert np.all(d["ti"] != 0) or e["nt"] >= 16, e["name"]
    print("the dearest entry: %s, %d multiply-adds" % max((cases.work(e), e["name"]) for e in ENTRIES)[::-1])
    # part C: np exact and padded by 1 .. 7 (Q15: even counts), odd and even step counts, filters shorter than the factor
    for f32 in (0, 1):
        mine = [e for e in ENTRIES if e["part"] == "C" and e["f32"] == f32]
        assert {e["D"] for e in mine} == {2, 3, 32} and all(e["nout"] == 130 for e in mine)
        assert {e["np"] - e["nt"] for e in mine} == ({0, 1, 2, 3} if f32 else {0, 2, 6})
        assert {(e["np"] // cases.QUANT[f32]) % 2 for e in mine} == {0, 1} and any(e["np"] < e["D"] for e in mine)
        assert {e["np"] // cases.QUANT[f32] for e in mine} >= {1, 2}


def test_part_d_is_the_setters_limit():
    part_d = [e for e in ENTRIES if e["part"] == "D"]
    assert [(e["f32"], e["D"], e["nt"]) for e in part_d] == [(0, 57, 256), (0, 58, 3968), (0, 60, 3840), (0, 32, 4096), (1, 59, 64), (1, 56, 256), (1, 32, 1792)]
    for e in part_d:
        q = cases.QUANT[e["f32"]]
        assert e["nt"] == e["np"] == min(max_taps(e["f32"], e["D"]), 4096) and e["refuse"] == e["nt"] + q, e["name"]
        beyond = fit(e["f32"], e["refuse"], e["D"], e["nout"])
        assert (beyond is None) == (e["nt"] < 4096), e["name"]           # one step up the rule refuses (or the interface does: 4096 taps)
        assert (e["cpw"], e["nw"], e["opl"]) == (1, 1, 2) and e["lowered"], e["name"]
        assert e["at_cap"] == (e["lds"] == 65536) == e["name"].endswith("-lds65536") == (e["nt"] < 4096), e["name"]
    assert max_taps(0, 32) == 5632 > 4096


@pytest.mark.parametrize("name", cases.names(1))
def test_fp32_bound_is_tight_and_the_output_is_not_degenerate(name):
    e = cases.BY_NAME[name]
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
    idx = cases.out_index(e)
    for c, (w, i, q) in enumerate(q15.refs_q15(oracle(), e)):
        assert np.abs(w[idx].astype(np.int32)).max() > 100, (name, c)
        assert np.abs(i[idx].astype(np.int32)).max() > 100 and np.abs(q[idx].astype(np.int32)).max() > 100, (name, c)
