"""The conditions on the table of the two-stage census (tests/pre_census_cases.py), checked without a GPU:

  * every entry's cpw, nw, opl, lds, tile and chunks are what the HEADER itself computes (a g++ probe over msdr_prepc_geometry.h), so the
    figures the GPU cases assert against chain.info() are the launcher's, not only the restated rule's; the same probe walks EVERY
    (D1, np1, np2, D2) the setters accept (np2 by bisection: the fit moves one way as np2 grows) and part A names exactly the keys it reaches;
  * part A holds all 30 (arithmetic, D1, CPW) triples, parts A and B together all 42 instantiations of tests/test_prefilter_pc_kernel.py's
    roster, part B every non-empty subset of {meter, pairs, gain}, an I/Q-only entry, a lowered one and one with AGC per arithmetic;
  * no entry asks more than 2e8 multiply-adds of the oracle, every stream is at least as long as both filters, every entry ends in a partial
    tile and has a partial channel group; parts C, D, E, F are what the table's docstring says, part D's figures the header's limits;
  * reference sanity per entry: Q15 audio and pairs exceed 100 on every channel; the fp32 model is within judge_f32's 2e-6 of float64 on
    every channel (e_orc, the oracle alone); and, in float64, zeroing the first or the last step (4 taps) of the prefilter row or of a channel
    pair moves some channel's audio by more than 1e-4 relative -- ten times the e_go clause --, so a kernel that drops such a step cannot pass."""
import os
import subprocess

import numpy as np
import pytest

import pre_census_cases as cases
import prefilter_model as pm
import test_gpu_pre_census as q15
import test_gpu_pre_census_f32 as fp32
from cx_cases import rel
from f32judge import oracle
from test_prefilter_pc_kernel import KERNELS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minimal-sdr_amd", "csrc")
ENTRIES = cases.ENTRIES
PROBE = r"""
#include <cstdio>
#include <set>
#include <tuple>
#include "msdr_prepc_geometry.h"
using namespace msdr;
static std::set<std::tuple<int, int, int, int, int, int>> keys;
static int al_of(int f, int D) { return f ? (D % 4 == 0 ? 4 : D % 2 == 0 ? 2 : 1) : ((D & 1) ? 0 : D % 8 == 0 ? 4 : D % 4 == 0 ? 2 : 1); }
static int fit_of(int f, long long nout, int np1, int D1, int np2, int D2)
{
    DecGeometry g;
    if (!pre_geometry(f == 1, nout, 1, 256, 0, np1, D1, np2, D2, &g)) return -1;
    keys.insert(std::make_tuple(f, nout <= 128 ? 4 : nout <= 256 ? 2 : 1, g.launch.cpw, g.nw, g.opl, al_of(f, D2)));
    return g.launch.cpw * 10000 + g.nw * 100 + g.opl;
}
// the LDS grows with np2 at every (cpw, nw, opl), so the first one that fits moves one way: equal ends mean an equal stretch
static void walk(int f, long long nout, int np1, int D1, int D2, int q, int lo, int a, int hi, int b)
{
    if (a == b || hi - lo <= q) return;
    const int mid = lo + (hi - lo) / (2 * q) * q, m = fit_of(f, nout, np1, D1, mid, D2);
    walk(f, nout, np1, D1, D2, q, lo, a, mid, m);
    walk(f, nout, np1, D1, D2, q, mid, m, hi, b);
}
int main()
{
    int f, D1, np1, np2, D2, ch; long long nout;
    while (scanf("%d %d %d %d %d %lld %d", &f, &D1, &np1, &np2, &D2, &nout, &ch) == 7) {
        DecGeometry g;
        if (!pre_geometry(f == 1, nout, ch, 256, 0, np1, D1, np2, D2, &g)) { printf("refused\n"); continue; }
        printf("%d %d %d %zu %d %u %u %d %d %d %d\n", g.launch.cpw, g.nw, g.opl, g.launch.lds_bytes, g.launch.tile, g.launch.block, g.launch.grid, g.launch.nseg,
               pre_chunks_per_tile(np2, D2, g.launch.tile, D1, g.launch.cpw), pre_max_taps(f == 1, D1, np2, D2), pre_max_decimation(f == 1, np1, D1, np2));
    }
    const int d1s[] = {2, 4, 8, 16, 32}, maxd[] = {60, 59};
    const long long nouts[] = {30, 130, 258};
    for (f = 0; f < 2; f++) {
        const int q = f ? 4 : 8;
        for (int d1 : d1s) for (int d2 = 1; d2 <= maxd[f]; d2++) for (long long n : nouts)
            for (int p1 = q; pre_fits(f == 1, p1, d1, q, d2); p1 += q) {
                int hi = 4096;
                while (hi > q && !pre_fits(f == 1, p1, d1, hi, d2)) hi -= q * ((hi - q) / (64 * q) + 1);          // (any fitting np2 near the top: walk() needs fitting ends)
                while (hi + q <= 4096 && pre_fits(f == 1, p1, d1, hi + q, d2)) hi += q;
                walk(f, n, p1, d1, d2, q, q, fit_of(f, n, p1, d1, q, d2), hi, fit_of(f, n, p1, d1, hi, d2));
            }
    }
    for (const auto &k : keys) printf("key %d %d %d %d %d %d\n", std::get<0>(k), std::get<1>(k), std::get<2>(k), std::get<3>(k), std::get<4>(k), std::get<5>(k));
    return 0;
}
"""


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    """(one line of figures per entry, the set of keys the header reaches)"""
    d = tmp_path_factory.mktemp("precensus")
    src, exe = str(d / "probe.cpp"), str(d / "probe")
    with open(src, "w") as f:
        f.write(PROBE)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + CSRC, "-o", exe, src])
    asked = "".join("%d %d %d %d %d %d %d\n" % (e["f32"], e["D1"], e["np1"], e["np2"], e["D2"], e["nout"], e["channels"]) for e in ENTRIES)
    lines = subprocess.run([exe], input=asked, check=True, capture_output=True, text=True).stdout.splitlines()
    keys = {tuple(int(v) for v in ln.split()[1:]) for ln in lines if ln.startswith("key")}
    return [ln for ln in lines if not ln.startswith("key")], keys


def test_every_entry_has_the_geometry_the_header_computes(probe):
    lines, _ = probe
    assert len(lines) == len(ENTRIES)
    for e, ln in zip(ENTRIES, lines):
        cpw, nw, opl, lds, tile, block, grid, nseg, chunks, max_taps, max_dec = (int(v) for v in ln.split())
        assert (cpw, nw, opl, lds, tile, block, chunks) == (e["cpw"], e["nw"], e["opl"], e["lds"], e["tile"], 64 * e["nw"], e["chunks"]), (e["name"], ln)
        assert nseg == e["nseg"] == (2 if e["part"] == "F" else 1), (e["name"], ln)
        groups = (e["channels"] + cpw - 1) // cpw
        assert groups == min(nw + 1, (17 + cpw - 1) // cpw) and grid == (groups * nseg + nw - 1) // nw, (e["name"], ln)          # a full workgroup and a single valid group
        assert grid == (2 if nseg == 1 else 3), (e["name"], ln)
        if e["limit"] == "taps":
            assert e["N1"] == e["np1"] == max_taps and e["refuse"] == max_taps + cases.QUANT[e["f32"]], (e["name"], ln)
        if e["limit"] == "factor":
            assert e["D2"] == min(max_dec, cases.MAX_D[e["f32"]]) and e["refuse"] == e["D2"] + 1 and max_dec < cases.MAX_D[e["f32"]], (e["name"], ln)


def test_part_a_is_every_reachable_geometry_behind_every_first_factor(probe):
    _, reached = probe
    part_a = [e for e in ENTRIES if e["part"] == "A"]
    keys = [cases.key(e) for e in part_a]
    assert len(set(keys)) == len(keys) and set(keys) == reached, (sorted(reached - set(keys)), sorted(set(keys) - reached))
    triples = {(e["f32"], e["D1"], e["cpw"]) for e in part_a}
    assert triples == {(f, d, c) for f in (0, 1) for d in cases.FACTORS for c in (1, 2, 4)} and len(triples) == 30
    lowered = [e for e in part_a if e["lowered"]]
    by_d1 = {d: sum(e["D1"] == d for e in part_a) for d in cases.FACTORS}
    print("reachable geometries: %d (Q15 %d, fp32 %d); the fit lowers CPW in %d; entries per D1 %s" % (len(keys), sum(not k[0] for k in keys), sum(k[0] for k in keys), len(lowered), by_d1))
    assert (len(keys), sum(not k[0] for k in keys), sum(k[0] for k in keys)) == (114, 69, 45)
    assert min(by_d1.values()) >= 15                                      # D1 = 16 among them: several entries each
    assert {(e["cls"], e["cpw"]) for e in lowered} == {(4, 2), (4, 1), (2, 1)}
    assert all(not e["full"] and e["N1"] == e["np1"] and e["N2"] == e["np2"] for e in part_a)
    # Q15 AL = 4 (D2 a multiple of 8) at every CPW
    assert {e["cpw"] for e in part_a if not e["f32"] and e["al"] == 4} == {1, 2, 4} and sum(1 for e in ENTRIES if not e["f32"] and e["al"] == 4) >= 15


def test_parts_a_and_b_name_all_42_instantiations():
    assert len(set(cases.NAMES)) == len(ENTRIES)
    named = {"chain_%spcn2_%skernelILi%dELi%dEE" % (cases.ARITH[f], "full_" if full else "", cpw, al)
             for f, full, cpw, al in {cases.instantiation(e) for e in ENTRIES if e["part"] in "AB"}}
    assert named == set(KERNELS) and len(named) == 42
    src = open(os.path.join(CSRC, "msdr_chain_pre.hip")).read()
    assert "(D & 1) ? 0 : (D % 8 == 0) ? 4 : (D % 4 == 0) ? 2 : 1" in src and "(D % 4 == 0) ? 4 : (D % 2 == 0) ? 2 : 1" in src
    assert "const bool full = p.meter || p.iq || p.agc;" in src
    for f32, pairs in ((0, 12), (1, 9)):
        mine = [e for e in ENTRIES if e["part"] == "B" and e["f32"] == f32]
        assert all(e["full"] for e in mine)
        assert len({(e["cpw"], e["al"]) for e in mine}) == pairs == len({(e["cpw"], e["al"]) for e in ENTRIES if e["part"] == "A" and e["f32"] == f32})
        assert {(e["meter"], e["iq"], e["gain"]) for e in mine if not e["agc"]} == set(cases.SUBSETS) and len(cases.SUBSETS) == 7
        assert sum(not e["out"] for e in mine) == 1 and all(e["iq"] for e in mine if not e["out"])
        assert sum(e["lowered"] for e in mine) >= 1 and sum(e["agc"] for e in mine) == 1
        assert len(mine) == pairs + 2
    counts = [sum(e["part"] == p for e in ENTRIES) for p in "ABCDEF"]
    print("parts A .. F: %s entries, %d in all (Q15 %d, fp32 %d)" % (counts, len(ENTRIES), len(cases.names(0)), len(cases.names(1))))
    assert counts == [114, 25, 52, 8, 5, 6] and len(ENTRIES) == 210


def test_the_recipe_and_the_cost_of_every_entry():
    tiles = {opl * 64 // cpw for opl in (2, 4, 8) for cpw in (1, 2, 4)}
    assert all(n % t for n in cases.LENGTHS.values() for t in tiles)      # every call ends in a partial tile
    for e in ENTRIES:
        assert cases.work(e) <= cases.WORK_CAP, (e["name"], cases.work(e))
        assert cases.is_covered(e), e["name"]
        assert e["channels"] == min(17, e["cpw"] * e["nw"] + 1) and e["channels"] % e["cpw"] == 1 % e["cpw"], e["name"]
        assert e["np1"] == cases.padded(e["f32"], e["N1"]) and e["np2"] == cases.padded(e["f32"], e["N2"]) and e["lds"] <= pm.CAP and e["D"] == e["D1"] * e["D2"], e["name"]
        assert e["nout"] % e["tile"] and (e["part"] == "F" or e["nout"] == cases.LENGTHS[e["cls"]]), e["name"]
        assert e["at_cap"] == (e["lds"] == 65536) and (e["part"] != "D" or e["at_cap"] == e["name"].endswith("-lds65536")), e["name"]
        d = cases.data(e)
        assert d["x"].shape == (e["channels"], cases.total(e)) and d["p"].size == e["N1"] and d["ti"].shape == (e["channels"], e["N2"]), e["name"]
        for row in (d["p"][None, :], d["ti"], d["tq"]):                  # (ripple and design may cancel on a coefficient of a long row; its oldest taps are ripple alone)
            assert (np.all(row != 0) or row.shape[1] >= 16) and np.all(np.any(row[:, :4] != 0, axis=1)) and np.all(np.any(row[:, -4:] != 0, axis=1)), e["name"]
    print("the dearest entry: %s, %d multiply-adds" % max((cases.work(e), e["name"]) for e in ENTRIES)[::-1])
    for f32 in (0, 1):
        q = cases.QUANT[f32]
        part_c = [e for e in ENTRIES if e["part"] == "C" and e["f32"] == f32]
        assert {e["D1"] for e in part_c} == {2, 16, 32} and all(e["nout"] == 130 and e["D2"] == 3 for e in part_c)
        for D1 in (2, 16, 32):
            assert {e["np1"] - e["N1"] for e in part_c if e["D1"] == D1} == (set(range(4)) if f32 else {0, 2, 4, 6}), (f32, D1)
            assert any(e["N1"] < D1 for e in part_c if e["D1"] == D1) or D1 == 2
        assert {e["np1"] // q for e in part_c} >= {1, 2} and {(e["np1"] // q) % 2 for e in part_c if e["np1"] > 2 * q} == {0, 1}          # odd and even step counts
        whole = [e for e in part_c if e["last"] == pm.chunk(e["D1"], e["cpw"])]
        assert any(e["D1"] == 16 and e["name"].endswith("whole-chunks") for e in whole)
        assert min(e["last"] for e in part_c) == q                        # the window is a multiple of the step: no shorter last chunk exists
        assert not f32 and all(e["al"] == 0 for e in part_c) or f32       # Q15: odd D2, two copies of the window (the second copy's w > 0 edge)
        part_d = [e for e in ENTRIES if e["part"] == "D" and e["f32"] == f32]
        assert [e["limit"] for e in part_d] == ["taps", "taps", "factor", "factor"] and any(e["at_cap"] for e in part_d)
        assert all((e["cpw"], e["opl"]) == (1, 2) or e["limit"] == "factor" for e in part_d)
        part_f = [e for e in ENTRIES if e["part"] == "F" and e["f32"] == f32]
        assert [(e["cpw"], e["opl"]) for e in part_f] == [(1, 2), (1, 4), (1, 8)] and all(e["nout"] == 8 * e["tile"] + 2 and e["calls"] == 1 for e in part_f)
        assert len({e["al"] for e in part_f}) >= 2
        for e in part_f:          # two segments of five tiles: the last tile of the second lies wholly past n_out
            g = pm.geometry(bool(f32), e["np1"], e["D1"], e["np2"], e["D2"], e["nout"], e["channels"], cases.CUS)
            assert g["nseg"] == 2 and g["seg_len"] == 5 * e["tile"] and 9 * e["tile"] >= e["nout"] > 8 * e["tile"], e["name"]
    part_e = [e for e in ENTRIES if e["part"] == "E"]
    assert [e["D1"] for e in part_e] == list(cases.FACTORS) and all(not e["f32"] and e["kind"] == "sat" for e in part_e)


@pytest.mark.parametrize("name", cases.names(0))
def test_q15_rows_are_not_degenerate(name):
    e = cases.BY_NAME[name]
    orc = oracle()
    audio, pairs, _ = q15.expected_q15(orc, e)
    for c in range(e["channels"]):
        assert np.abs(audio[c].astype(np.int32)).max() > 100, (name, c)
        assert np.abs(pairs[c, :, 0].astype(np.int32)).max() > 100, (name, c)
        assert np.abs(pairs[c, :, 1].astype(np.int32)).max() > 100 if e["kind"] != "sat" else not pairs[c, :, 1].any(), (name, c)          # (part E: sin = 0)
    if e["kind"] == "sat":
        assert all(q15.rails_and_wrap(orc, e).values()), name


def _zeroed(a, first, step=4):
    a = np.array(a)
    if first:
        a[..., :step] = 0
    else:
        a[..., -step:] = 0
    return a


@pytest.mark.parametrize("name", cases.names(1))
def test_fp32_oracle_is_inside_the_judges_bound_and_every_edge_step_matters(name):
    e = cases.BY_NAME[name]
    d = cases.data(e)
    si, sq = q15.osc(e)
    worst = 0.0
    for c, (want, truth) in enumerate(fp32.refs_f32(oracle(), e)):
        for stream, w, t in zip(("audio", "fi", "fq"), want, truth):
            e_orc = rel(w, t)
            worst = max(worst, e_orc)
            assert e_orc < 2e-6, (name, c, stream, e_orc)
        assert float(np.sqrt((truth[0] ** 2).mean())) > 1e-3, (name, c)
    print("%s worst e_orc %.3e" % (name, worst))
    # teeth: the first / the last step of the prefilter row, of the channel pair, zeroed in float64 (the row as the kernel holds it: padded in front)
    front = np.zeros(e["np1"] - e["N1"], d["p"].dtype)
    p = np.concatenate([front, d["p"]])
    pad2 = np.zeros((e["channels"], e["np2"] - e["N2"]), d["ti"].dtype)
    ti, tq = np.concatenate([pad2, d["ti"]], axis=1), np.concatenate([pad2, d["tq"]], axis=1)
    for what in ("prefilter first", "prefilter last", "channel first", "channel last"):
        first = what.endswith("first")
        moved = 0.0
        for c, (_, truth) in enumerate(fp32.refs_f32(oracle(), e)):
            if what.startswith("prefilter"):
                got = pm.model_f64(d["x"][c], si[c], sq[c], _zeroed(p, first), e["D1"], d["modes"][c], ti[c], tq[c], e["D2"])[0]
            else:
                got = pm.model_f64(d["x"][c], si[c], sq[c], p, e["D1"], d["modes"][c], _zeroed(ti[c], first), _zeroed(tq[c], first), e["D2"])[0]
            moved = max(moved, rel(got, truth[0]))
            if moved > 1e-4:
                break
        print("%s %s step zeroed: relative error %.3e" % (name, what, moved))
        assert moved > 1e-4, (name, what, moved)
