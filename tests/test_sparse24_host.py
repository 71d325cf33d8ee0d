"""minimal-sdr_amd/csrc/msdr_sparse24.h on the CPU (tests/cpp/test_sparse24.cpp, a stand-alone program built with g++ under the address and
undefined-behaviour sanitizers): a run's first and last tap block merged into one 2:4-sparse operand and expanded again by the documented
encoding is the K-stacked pair exactly, in both fp16 pieces -- banded Toeplitz blocks (bands of 8, 52, 128 and 256 samples per parity, both band
starts) and random complementary blocks; overlapping blocks are refused; index pairs increase strictly.  Built with -DMSDR_MUTATE=1 / =2 the
same program holds the mutated split: `make mutants` acts on the merged pieces as on the dense fragments."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_sparse24.cpp")


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ missing")
@pytest.mark.parametrize("mutate", [0, 1, 2])
def test_merge_expands_to_the_stacked_pair(tmp_path, mutate):
    exe = str(tmp_path / ("test_sparse24_%d" % mutate))
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    cmd += ["-DMSDR_MUTATE=%d" % mutate] if mutate else []
    r = subprocess.run(cmd + ["-o", exe, SRC], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and "(MSDR_MUTATE %d): 0 failures" % mutate in r.stdout, r.stdout[-3000:]
