"""The K-stacked A operands of the folded cascade's two sparse matrix products (minimal-sdr_amd/csrc/msdr_kstack.h: R sigma and Rd delta as
[X_hi | X_hi ; X_lo] . [v_hi ; v_lo ; v_hi], the three split-fp16 terms summed by one matrix instruction's own K reduction), checked on the
host by tests/cpp/kstack_check.hip, which includes the header as it is and launches nothing: the 16-row K sum in double equals
X_hi v_hi + X_hi v_lo + X_lo v_hi for the two-instruction and for the one-instruction form.  Built a second time with -DMSDR_MUTATE=5 (the
mutant tests/test_gpu_f32_teeth.py runs on the GPU) the X_lo v_hi term is gone and nothing else changes: the X_hi entries of both builds
carry the same checksum."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SRC = os.path.join(ROOT, "tests", "cpp", "kstack_check.hip")


def build_and_run(tmp_path, name, defines, args):
    exe = str(tmp_path / name)
    r = subprocess.run([HIPCC, "--offload-host-only", "-O1", "-std=c++17", "-Wall"] + defines + ["-o", exe, SRC],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([exe] + args, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and ": 0 failures" in r.stdout, r.stdout[-3000:]
    return int(re.search(r"hi-checksum (\d+)", r.stdout).group(1))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc missing")
def test_stacked_operands_sum_to_the_three_split_terms(tmp_path):
    product = build_and_run(tmp_path, "kstack_check", [], [])
    mutant = build_and_run(tmp_path, "kstack_check_mut5", ["-DMSDR_MUTATE=5"], ["mutant"])
    assert product == mutant, "MSDR_MUTATE=5 changed entries that hold X_hi"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc missing")
def test_the_check_sees_a_missing_lo_term(tmp_path):
    """The mutant's tables against the product's expectation: the check fails (it has teeth)."""
    exe = str(tmp_path / "kstack_check_mut5")
    r = subprocess.run([HIPCC, "--offload-host-only", "-O1", "-std=c++17", "-Wall", "-DMSDR_MUTATE=5", "-o", exe, SRC],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 1 and ": 0 failures" not in r.stdout, r.stdout[-3000:]
