"""The census table of the Q15 serial-recurrence ladders (tests/q15_ladder_cases.py), checked without a GPU against the library's SOURCE:

  * coverage of kernels: every __global__ kernel of csrc/ named biquad_teensy* / frontend*, in every template instantiation the host launches
    (read out of the hipLaunchKernelGGL lines and launcher switches of msdr_api.hip / msdr_biquad_pc.hip), is the expected kernel of an entry or
    is listed UNREACHABLE with its reason -- a kernel added later without an entry turns this red here, on the CPU;
  * coverage of edges: both sides of every ladder condition have an entry, and the two differ in that condition only;
  * census identity: the names the census expects are exactly the strings the three getters can return (the literals of the source), and the
    launch's error check is handed the same pointer, so the name cannot drift from the launch;
  * the expectation function (written from include/msdr.h's rules) gives every entry's kernel for every call length and every CU count."""
import os
import re

import pytest

import q15_ladder_cases as census

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "minimal-sdr_amd", "csrc")
PATTERN = r"(?:biquad_teensy|frontend)\w*"


def _read(name):
    return open(os.path.join(CSRC, name)).read()


def _no_comments(src):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))


def defined_kernels():
    """{kernel name: is a template} over every file of csrc/"""
    out = {}
    for f in sorted(os.listdir(CSRC)):
        if not f.endswith((".hip", ".hiph", ".h", ".cpp")):
            continue
        src = _no_comments(_read(f))
        for m in re.finditer(r"(template\s*<[^>]*>\s*)?(?:static\s+)?__global__[^;{]*?\bvoid\s+(%s)\s*\(" % PATTERN, src):
            out[m.group(2)] = bool(m.group(1))
    return out


def launched_instances():
    """every instantiation the host launches, as the getters spell it: name<args> without blanks"""
    src = _no_comments(_read("msdr_api.hip")) + _no_comments(_read("msdr_biquad_pc.hip"))
    macro_args = {"CH_": sorted(set(re.findall(r"MSDR_(?:TQ4|FE4)_LAUNCH\((\d+)\)", src)))}
    assert macro_args["CH_"] == ["16", "32", "64"], macro_args
    # (the two macros take the same three values: checked one by one)
    assert sorted(re.findall(r"MSDR_TQ4_LAUNCH\((\d+)\)", src)) == ["16", "32", "64"] and sorted(re.findall(r"MSDR_FE4_LAUNCH\((\d+)\)", src)) == ["16", "32", "64"]
    out = set()
    for m in re.finditer(r"hipLaunchKernelGGL\(\s*\(?\s*(%s)\s*(<[^>]*>)?" % PATTERN, src):
        name, args = m.group(1), (m.group(2) or "").replace(" ", "")
        if "CH_" in args:
            out |= {name + args.replace("CH_", v) for v in macro_args["CH_"]}
        else:
            out.add(name + args)
    return out


def getter_literals():
    """every string the three getters can return: the literals assigned to last_kernel / node_kname in msdr_api.hip, macro arguments expanded"""
    src = _no_comments(_read("msdr_api.hip"))
    out = set()
    for m in re.finditer(r"\b(?:last_kernel|node_kname|node_kernel)\s*=\s*((?:\"[^\"]*\"|#CH_|\s)+);", src):
        parts = re.findall(r"\"([^\"]*)\"|(#CH_)", m.group(1))
        if any(p[1] for p in parts):
            out |= {"".join(v if arg else lit for lit, arg in parts) for v in ("16", "32", "64")}
        else:
            out.add("".join(p[0] for p in parts))
    return out


def test_entries_are_well_formed():
    assert len(set(census.NAMES)) == len(census.NAMES)
    for e in census.ENTRIES:
        assert e["ladder"] in ("chain", "node", "frontend"), e["name"]
        assert len(e["lengths"]) >= 3, e["name"]                                   # state is carried at least twice
        assert e["channels"] <= 4112 and max(e["lengths"]) <= 384, e["name"]
        assert all(n % 2 == 0 for n in e["lengths"]), e["name"]                    # AudioFilterBiquad processes sample pairs
        if e["ladder"] == "frontend":
            assert all(n % 128 == 0 for n in e["lengths"]) and not e["nodes"], e["name"]
        if e["ladder"] == "node":
            assert len(e["nodes"]) == 1, e["name"]
        if e["block_kernel"]:
            assert e["pc_taps"], e["name"]


@pytest.mark.parametrize("cu_count", [8, 32, 64, 128, 256])
def test_expectation_function_gives_every_entrys_kernel(cu_count):
    for e in census.ENTRIES:
        for n in e["lengths"]:
            assert census.expected(e, n, cu_count) == e["kernel"], (e["name"], n, cu_count)


def test_every_kernel_and_every_launched_instance_is_accounted_for():
    defined, launched = defined_kernels(), launched_instances()
    assert set(defined) == {"biquad_teensy_kernel", "biquad_teensy_pipe_kernel", "biquad_teensy_pipe4_kernel", "biquad_teensy_blk_kernel", "biquad_teensy_pc_kernel",
                            "frontend_kernel", "frontend_pipe4_kernel"} | {k.split("<")[0] for k in census.UNREACHABLE}, sorted(defined)
    # what the switches are read as: two NODES for each of the lane kernels, 2 x 3 and 3 slab pipelines, the three without arguments
    assert launched == {"biquad_teensy_kernel<1>", "biquad_teensy_kernel<2>", "biquad_teensy_pc_kernel<1>", "biquad_teensy_pc_kernel<2>", "biquad_teensy_pipe_kernel",
                        "biquad_teensy_blk_kernel", "frontend_kernel"} | {"biquad_teensy_pipe4_kernel<%d,%d>" % (nd, c) for nd in (1, 2) for c in (16, 32, 64)} \
        | {"frontend_pipe4_kernel<%d>" % c for c in (16, 32, 64)} | {k for k in census.UNREACHABLE if k in launched}, sorted(launched)
    for k, is_template in defined.items():          # a kernel nobody launches is dead code: it is launched, or listed with its reason
        assert any(inst.split("<")[0] == k for inst in launched) or any(u.split("<")[0] == k for u in census.UNREACHABLE), k
        assert all(("<" in inst) == is_template for inst in launched if inst.split("<")[0] == k), k
    have = {e["kernel"] for e in census.ENTRIES}
    missing = sorted(k for k in launched if k not in have and k not in census.UNREACHABLE)
    assert missing == [], missing
    for k, why in census.UNREACHABLE.items():
        assert k not in have and len(why) > 20, k


def test_census_names_are_exactly_what_the_getters_can_return():
    lits = getter_literals()
    assert "" in lits
    mine = {e["kernel"] for e in census.ENTRIES}
    assert mine == lits, (sorted(lits - mine), sorted(mine - lits))
    assert len(lits) == 19, sorted(lits)
    # every launch of the three ladders hands its error check the recorded pointer: no literal of these names is left in a launch_check
    src = _no_comments(_read("msdr_api.hip"))
    assert re.findall(r"launch_check\(\"(?:%s)[^\"]*\"\)" % PATTERN, src) == []
    assert len(re.findall(r"launch_check\((?:S->last_kernel|fe->last_kernel|node_kname)\)", src)) == 6
    hdr = open(os.path.join(ROOT, "include", "msdr.h")).read()
    for k in lits - {""}:
        generic = re.sub(r"\d+>$", "P>", k) if "pipe4" in k else k
        assert '"%s"' % generic in hdr, k          # the header's table of the ladders names every one of them


def test_both_sides_of_every_condition_have_an_entry():
    own = ("name", "kernel", "note")
    for ladder, cond, a, b, fields in census.EDGES:
        ea, eb = census.BY_NAME[a], census.BY_NAME[b]
        assert ea["ladder"] == eb["ladder"] == ladder, (cond, a, b)
        assert ea["kernel"] != eb["kernel"], (cond, a, b)
        differ = tuple(k for k in ea if k not in own and ea[k] != eb[k])
        assert differ == fields, (cond, a, b, differ)
    for cond, ladders in census.CONDITIONS.items():
        for ladder in ladders:
            assert any(l == ladder and c.startswith(cond) for l, c, *_ in census.EDGES), (cond, ladder)
    # the alignment edges are tried at both a 2-byte and an 8-byte offset where the kernels load 16 bytes from a row of 2-byte samples
    for ladder in ("chain", "node"):
        offs = {census.BY_NAME[b]["align"] for l, c, a, b, f in census.EDGES if l == ladder and f == ("align",)}
        assert {2, 8} <= offs, (ladder, offs)
    edged = {n for _, _, a, b, _ in census.EDGES for n in (a, b)}
    assert len(edged) >= 45
