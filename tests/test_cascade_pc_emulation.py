"""biquad_df1_seq_pc_kernel's own text run on the CPU (tests/cpp/cascade_pc_emu.cpp): one thread per lane, under the address and
undefined-behaviour sanitizers, against the plain sequential cascade -- indexing, bounds and bit-identity of every path, without a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_kernel_text_on_the_cpu_under_sanitizers(tmp_path):
    cxx = shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    if not os.path.exists(cxx):
        pytest.fail("clang++ not found (the kernel's vector types need it)")
    src = open(os.path.join(ROOT, "minimal-sdr_amd", "csrc", "msdr_biquad_df1_pc.hiph")).read()
    body = src[src.index("template <int S, bool SEG>"):src.rindex("}  // namespace msdr")]
    assert "biquad_df1_seq_pc_kernel" in body and "sbq_section" in body
    (tmp_path / "cascade_pc_kernel_body.inc").write_text(body)
    exe = str(tmp_path / "cascade_pc_emu")
    subprocess.check_call([cxx, "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-pthread",
                           "-I", str(tmp_path), "-o", exe, os.path.join(ROOT, "tests", "cpp", "cascade_pc_emu.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0 and "ALL OK" in r.stdout
