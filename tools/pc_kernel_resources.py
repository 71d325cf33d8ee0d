#!/usr/bin/env python3
"""Resource table of the per-receiver chain kernels, without a GPU: compiles their seven translation units to gfx950 assembly with the
Makefile's flags and prints, per instantiation, the code-object metadata and the instruction count of the body as a markdown table.

    python tools/pc_kernel_resources.py [--csrc DIR] [--against DIR]

--against: a second csrc directory (e.g. of the parent commit); its figures are printed beside these as the parent's and differences are marked."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")          # as the Makefile's HIPCC ?=
UNITS = ["msdr_chain_q15pc", "msdr_chain_f32pc", "msdr_chain_oscpc", "msdr_chain_ncopc", "msdr_chain_decpc", "msdr_chain_f32pcb", "msdr_chain_q15pcb"]
FIELDS = ["vgpr_count", "sgpr_count", "agpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count"]


def flags():
    mk = open(os.path.join(ROOT, "minimal-sdr_amd", "Makefile")).read()
    cxx = re.search(r"^CXXFLAGS := (.*)$", mk, re.M).group(1).split()
    hip = [f for f in re.search(r"^HIPFLAGS := (.*)$", mk, re.M).group(1).split() if not f.startswith("$(") and not f.startswith("--offload-arch")]
    return cxx + hip


def demangle(name):          # _ZN4msdr18chain_q15pc_kernelILi4ELb1EEEvNS_8PcParamsE -> chain_q15pc_kernel<4, true>
    m = re.match(r"_ZN4msdr\d+(chain_\w+?_kernel)I((?:L[ib]\d+E)+)E", name)
    if not m:
        return None          # (a static kernel of msdr_kernels.hiph that every unit carries)
    args = [("true" if v == "1" else "false") if t == "b" else v for t, v in re.findall(r"L([ib])(\d+)E", m.group(2))]
    return "%s<%s>" % (m.group(1), ", ".join(args))


def kernels(csrc):
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for u in UNITS:
            s = os.path.join(d, u + ".s")
            r = subprocess.run([HIPCC, "--offload-arch=gfx950"] + flags() + ["-S", "--cuda-device-only", "-o", s, os.path.join(csrc, u + ".hip")], stderr=subprocess.PIPE, text=True)
            if r.returncode:
                sys.exit("%s does not compile:\n%s" % (u, r.stderr))
            asm = open(s).read()
            for block in re.split(r"\n\s+- \.agpr_count:", "\n" + asm[asm.index("amdhsa.kernels"):])[1:]:
                block = ".agpr_count:" + block
                name = re.search(r"\.name:\s+(\S+)", block).group(1)
                if not demangle(name):
                    continue
                body = asm[asm.index("\n%s:" % name):]
                body = body[:body.index("s_endpgm")]
                insts = sum(1 for ln in body.splitlines() if re.match(r"\s+[a-z]\w+", ln) and not ln.lstrip().startswith((".", ";")))
                out[demangle(name)] = [int(re.search(r"\.%s:\s+(\d+)" % f, block).group(1)) for f in FIELDS] + [insts + 1]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=os.path.join(ROOT, "minimal-sdr_amd", "csrc"))
    ap.add_argument("--against")
    a = ap.parse_args()
    new, old = kernels(a.csrc), kernels(a.against) if a.against else None
    cols = ["vgpr", "sgpr", "agpr", "lds", "private", "spills", "instructions"]
    print("| kernel | " + " | ".join(cols) + (" | vgpr allocation (this / parent) | body |" if old else " |"))
    print("|---" * (len(cols) + (3 if old else 1)) + "|")
    for k in sorted(new):
        row = "| `%s` | " % k + " | ".join(str(v) for v in new[k])
        if old and k not in old:          # an instantiation the parent does not have (e.g. the metered flavours)
            row += " | %d / - | new" % ((new[k][0] + 7) // 8 * 8)
        elif old:
            o = old[k]
            diff = ", ".join("%s %d -> %d" % (c, ov, nv) for c, ov, nv in zip(cols, o, new[k]) if ov != nv)
            row += " | %d / %d | %s" % ((new[k][0] + 7) // 8 * 8, (o[0] + 7) // 8 * 8, "same figures" if not diff else "parent -> this: " + diff)
        print(row + " |")


if __name__ == "__main__":
    main()
