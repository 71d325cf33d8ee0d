"""The wave-stream envelope kernels with a constant run geometry (chain_mfw_geom_kernel<RL, MwGeom<...>>, minimal-sdr_amd/csrc/msdr_chain_mfw.hiph)
exist to take the instructions out of the FIR burst that only serve run-time geometry: scalars parked in VGPR lanes and read back
(v_readlane_b32), address adds, the loop and its branches, the accumulator copy in front of the merged step.  This test disassembles the
PRODUCT binary, as tests/test_chain_kernel_no_scratch.py does, and holds every specialised kernel to that: in every stretch from
`s_setprio 3` to the next `s_setprio 1` (the burst of the hot and of the cold tile) no read-lane, no branch, exactly the matrix
instructions of the geometry named by the kernel's own template arguments (3 per dense step, 3 v_smfmac per merged run) and no more
register moves than the merged steps' operand interleave needs (14 each; the compiler is allowed two more).  No scratch instruction, 4
waves per SIMD.  The run-time twin in the same binary (chain_mfw_rowlocal_kernel) is the control: its burst does hold read-lanes and
branches, so the assertions have something to lose.  No GPU needed."""
import os
import re
import subprocess

import pytest

from test_chain_kernel_no_scratch import LIB, OBJDUMP, READELF, code_object, kernels_of

GEOM = re.compile(r"chain_mfw_geom_kernelILi(\d)ENS_6MwGeomILi(\d+)ELi(\d+)E" + r"Li(\d+)ELi(\d+)ELb([01])E" * 4 + r"Li(\d+)E")


def geometry_of(name):
    """The template arguments in a mangled name: RL, id, halo, four runs (j0, cnt, merged), acc1_base."""
    m = GEOM.search(name)
    assert m, name
    g = [int(v) for v in m.groups()]
    runs = [tuple(g[3 + 3 * k:6 + 3 * k]) for k in range(4)]
    return dict(rl=g[0], id=g[1], halo=g[2], runs=runs, acc1_base=g[15])


def bursts(ins):
    out, cur = [], None
    for i in ins:
        if i.startswith("s_setprio 3"):
            cur = []
        elif cur is not None and i.startswith("s_setprio 1"):
            out.append(cur)
            cur = None
        elif cur is not None:
            cur.append(i)
    return out


def count(ins, *prefixes):
    return sum(1 for i in ins if i.startswith(prefixes))


@pytest.fixture(scope="module")
def disassembly(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("mfw_geom"))
    cos = code_object(tmp)
    text = "\n".join(subprocess.run([OBJDUMP, "-d", co], check=True, stdout=subprocess.PIPE, text=True).stdout for co in cos)
    notes = "\n".join(subprocess.run([READELF, "--notes", co], check=True, stdout=subprocess.PIPE, text=True).stdout for co in cos)
    return text, notes


needs_tools = pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(OBJDUMP) and os.path.exists(READELF)), reason="library or llvm tools missing")


@needs_tools
def test_the_burst_of_every_specialised_kernel_is_straight_line_code_with_its_geometrys_products(disassembly):
    kernels = kernels_of(disassembly[0], "chain_mfw_geom_kernel")
    geoms = {k: geometry_of(k) for k in kernels}
    # both row-local variants of the 256-tap (halo 288) and of the 512-tap (halo 544) envelope geometry
    assert sorted((g["rl"], g["id"], g["halo"]) for g in geoms.values()) == [(1, 1, 288), (1, 2, 544), (2, 1, 288), (2, 2, 544)], sorted(kernels)
    for name, ins in kernels.items():
        g = geoms[name]
        dense = sum(cnt - 2 * mg for _, cnt, mg in g["runs"])
        merged = sum(mg for _, cnt, mg in g["runs"])
        assert merged == 2 and dense == 2 * (g["halo"] // 32 - 2), (name, g)
        assert not [i for i in ins if i.startswith("scratch_")], name
        bs = bursts(ins)
        assert len(bs) == 2, (name, len(bs))                                  # the hot and the cold tile
        for b in bs:
            got = dict(readlane=count(b, "v_readlane_b32"), writelane=count(b, "v_writelane_b32"), branch=count(b, "s_cbranch", "s_branch"),
                       mfma=count(b, "v_mfma_"), smfmac=count(b, "v_smfmac_"), mov=count(b, "v_mov_"))
            print(name[:60], g["id"], got, "of", len(b), "instructions")
            assert got["readlane"] == 0 and got["writelane"] == 0 and got["branch"] == 0, (name, got)
            assert got["mfma"] == 3 * dense and got["smfmac"] == 3 * merged, (name, got, dense, merged)
            assert got["mov"] <= 14 * merged + 2, (name, got)


@needs_tools
def test_the_run_time_twin_does_hold_what_the_specialised_kernels_lost(disassembly):
    kernels = kernels_of(disassembly[0], "chain_mfw_rowlocal_kernel")
    assert len(kernels) == 2, sorted(kernels)
    for name, ins in kernels.items():
        bs = bursts(ins)
        assert bs, name
        b = max(bs, key=len)
        got = dict(readlane=count(b, "v_readlane_b32"), branch=count(b, "s_cbranch", "s_branch"), mov=count(b, "v_mov_"))
        print(name, got, "of", len(b), "instructions")
        assert got["readlane"] > 0 and got["branch"] > 0 and got["mov"] > 14 * 2 + 2, (name, got)


@needs_tools
def test_every_specialised_kernel_keeps_four_waves_per_simd(disassembly):
    seen = 0
    for block in disassembly[1].split(".name:")[1:]:
        if "chain_mfw_geom_kernel" not in block.split()[0]:
            continue
        f = {k: int(v) for k, v in re.findall(r"\.(vgpr_count|agpr_count|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count):\s+(\d+)", block)}
        seen += 1
        assert f["vgpr_count"] + f.get("agpr_count", 0) <= 128 and f["private_segment_fixed_size"] == 0 and f.get("vgpr_spill_count", 0) == 0, (block.split()[0], f)
    assert seen == 4, seen
